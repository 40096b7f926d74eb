/*
 * obx_project.h — what the filtered-projection kernels (obx_project.hip) and
 * their host verb (obx_gpu_scan_project, obx_engine.cpp) share.
 */
#ifndef OBX_PROJECT_H_
#define OBX_PROJECT_H_

#include "obx_dev.h"

/* counts per workgroup of the block-offset scan (256 threads x 8) */
#define OBX_PROJ_TILE 2048

/* the projection list of one k_project_sel launch, passed by value: no
   device scratch, no upload before the launch */
typedef struct proj_args {
  uint8_t *out[OBX_DEV_MAX_COLS]; /* dense datum vector per position */
  uint16_t col[OBX_DEV_MAX_COLS];
  uint8_t len[OBX_DEV_MAX_COLS];  /* datum byte length */
  uint32_t n_proj;
} proj_args;

#endif /* OBX_PROJECT_H_ */
