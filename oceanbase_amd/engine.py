"""MI355X product engine bindings (oceanbase_amd/libobx.so, HIP/gfx950).

This is the PRODUCT path. It requires the in-tree HIP library; if the library
is missing or no GPU is present, calls raise — there is no CPU fallback (the
oracle is test infrastructure only).
"""
import ctypes as C
import os

from . import abi

_PKG = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_PKG, "libobx.so")

OBX_NO_GPU = -7001


class EngineUnavailable(RuntimeError):
    pass


def _load():
    if not os.path.exists(_SO):
        raise EngineUnavailable(
            f"{_SO} not built — run oceanbase_amd/csrc/build.sh (the product "
            "path has no CPU fallback)")
    lib = C.CDLL(_SO)
    lib.obx_gpu_open.restype = C.c_int
    lib.obx_gpu_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.obx_gpu_close.restype = C.c_int
    lib.obx_gpu_close.argtypes = [C.c_void_p]
    lib.obx_gpu_load_blocks.restype = C.c_int
    lib.obx_gpu_load_blocks.argtypes = [C.c_void_p, C.POINTER(abi.BlockSet)]
    lib.obx_gpu_load_cs_blocks.restype = C.c_int
    lib.obx_gpu_load_cs_blocks.argtypes = [C.c_void_p,
                                           C.POINTER(abi.BlockSet)]
    lib.obx_gpu_free_blocks.restype = C.c_int
    lib.obx_gpu_free_blocks.argtypes = [C.c_void_p, C.c_int]
    lib.obx_gpu_filter.restype = C.c_int
    lib.obx_gpu_filter.argtypes = [C.c_void_p, C.c_int,
                                   C.POINTER(abi.FilterDesc), C.c_int]
    lib.obx_gpu_fetch_bitmap.restype = C.c_int
    lib.obx_gpu_fetch_bitmap.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_int64]
    lib.obx_gpu_fetch_row_ids.restype = C.c_int
    lib.obx_gpu_fetch_row_ids.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_int64, C.POINTER(C.c_uint64)]
    lib.obx_gpu_fetch_blk_counts.restype = C.c_int
    lib.obx_gpu_fetch_blk_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_int64]
    lib.obx_gpu_decode.restype = C.c_int
    lib.obx_gpu_decode.argtypes = [C.c_void_p, C.c_int,
                                   C.POINTER(C.c_uint16), C.c_uint16]
    lib.obx_gpu_fetch_col.restype = C.c_int
    lib.obx_gpu_fetch_col.argtypes = [C.c_void_p, C.c_int, C.c_uint16,
                                      C.c_void_p, C.c_int64]
    lib.obx_gpu_scan_project.restype = C.c_int
    lib.obx_gpu_scan_project.argtypes = [C.c_void_p, C.c_int,
                                         C.POINTER(abi.FilterDesc),
                                         C.POINTER(C.c_uint16), C.c_uint16,
                                         C.c_int, C.POINTER(C.c_uint64)]
    lib.obx_gpu_fetch_proj.restype = C.c_int
    lib.obx_gpu_fetch_proj.argtypes = [C.c_void_p, C.c_int, C.c_uint16,
                                       C.c_uint64, C.c_uint64, C.c_void_p,
                                       C.c_int64, C.c_void_p, C.c_int64,
                                       C.POINTER(C.c_uint64)]
    lib.obx_gpu_fetch_proj_row_nos.restype = C.c_int
    lib.obx_gpu_fetch_proj_row_nos.argtypes = [C.c_void_p, C.c_int,
                                               C.c_uint64, C.c_uint64,
                                               C.c_void_p, C.c_int64,
                                               C.POINTER(C.c_uint64)]
    lib.obx_gpu_last_proj_stage_ms.restype = C.c_double
    lib.obx_gpu_last_proj_stage_ms.argtypes = [C.c_void_p, C.c_int]
    lib.obx_gpu_scan_filter_agg.restype = C.c_int
    lib.obx_gpu_scan_filter_agg.argtypes = [C.c_void_p, C.c_int,
                                            C.POINTER(abi.FilterDesc),
                                            C.POINTER(abi.AggDesc),
                                            C.POINTER(abi.AggResult)]
    lib.obx_gpu_last_kernel_ms.restype = C.c_double
    lib.obx_gpu_last_kernel_ms.argtypes = [C.c_void_p]
    lib.obx_gpu_last_prep_ms.restype = C.c_double
    lib.obx_gpu_last_prep_ms.argtypes = [C.c_void_p]
    lib.obx_gpu_last_jit.restype = C.c_int
    lib.obx_gpu_last_jit.argtypes = [C.c_void_p]
    lib.obx_gpu_last_bdesc.restype = C.c_int
    lib.obx_gpu_last_bdesc.argtypes = [C.c_void_p]
    lib.obx_gpu_last_joint.restype = C.c_int
    lib.obx_gpu_last_joint.argtypes = [C.c_void_p]
    lib.obx_gpu_bdesc_builds.restype = C.c_int64
    lib.obx_gpu_bdesc_builds.argtypes = [C.c_void_p, C.c_int]
    lib.obx_gpu_keyset_create.restype = C.c_int
    lib.obx_gpu_keyset_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_int]
    lib.obx_gpu_keyset_from_proj.restype = C.c_int
    lib.obx_gpu_keyset_from_proj.argtypes = [C.c_void_p, C.c_int, C.c_uint16,
                                             C.c_int]
    lib.obx_gpu_keyset_free.restype = C.c_int
    lib.obx_gpu_keyset_free.argtypes = [C.c_void_p, C.c_int]
    lib.obx_gpu_keyset_info.restype = C.c_int
    lib.obx_gpu_keyset_info.argtypes = [C.c_void_p, C.c_int,
                                        C.POINTER(abi.KeysetInfo)]
    lib.obx_gpu_keyset_host_model.restype = C.c_int
    lib.obx_gpu_keyset_host_model.argtypes = [
        C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
        C.POINTER(abi.KeysetInfo)]
    lib.obx_gpu_keymap_create.restype = C.c_int
    lib.obx_gpu_keymap_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint64,
                                          C.POINTER(abi.ColSchema), C.c_int]
    lib.obx_gpu_keymap_from_proj.restype = C.c_int
    lib.obx_gpu_keymap_from_proj.argtypes = [C.c_void_p, C.c_int, C.c_uint16,
                                             C.c_uint16, C.c_int]
    lib.obx_gpu_keymap_free.restype = C.c_int
    lib.obx_gpu_keymap_free.argtypes = [C.c_void_p, C.c_int]
    lib.obx_gpu_keymap_info.restype = C.c_int
    lib.obx_gpu_keymap_info.argtypes = [C.c_void_p, C.c_int,
                                        C.POINTER(abi.KeymapInfo)]
    lib.obx_gpu_keymap_host_model.restype = C.c_int
    lib.obx_gpu_keymap_host_model.argtypes = [
        C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(abi.ColSchema), C.c_int,
        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
        C.POINTER(abi.KeymapInfo)]
    lib.obx_gpu_scan_join_agg.restype = C.c_int
    lib.obx_gpu_scan_join_agg.argtypes = [C.c_void_p, C.c_int,
                                          C.POINTER(abi.FilterDesc),
                                          C.POINTER(abi.JoinDesc),
                                          C.POINTER(abi.AggDesc),
                                          C.POINTER(abi.AggResult)]
    lib.obx_gpu_set_max_groups.restype = C.c_int
    lib.obx_gpu_set_max_groups.argtypes = [C.c_void_p, C.c_uint64]
    lib.obx_gpu_max_groups.restype = C.c_uint64
    lib.obx_gpu_max_groups.argtypes = [C.c_void_p]
    lib.obx_gpu_last_group_slots.restype = C.c_uint64
    lib.obx_gpu_last_group_slots.argtypes = [C.c_void_p]
    lib.obx_gpu_last_group_ms.restype = C.c_double
    lib.obx_gpu_last_group_ms.argtypes = [C.c_void_p]
    lib.obx_gpu_group_hash_host_model.restype = C.c_int
    lib.obx_gpu_group_hash_host_model.argtypes = [
        C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for f in ("obx_gpu_total_rows", "obx_gpu_total_bytes",
              "obx_gpu_last_survivors"):
        getattr(lib, f).restype = C.c_uint64
        getattr(lib, f).argtypes = [C.c_void_p, C.c_int]
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


class KeysetError(RuntimeError):
    """A key-set verb failed; .rc is the engine's status code."""

    def __init__(self, what, rc):
        super().__init__(f"{what} failed: {rc}")
        self.rc = rc


def _i64(a):
    import numpy as np
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64))


def keyset_host_model(keys, probe=(), kind=0):
    """TEST INFRASTRUCTURE: build a key set in host memory with the inline
    functions the device runs and probe it. Needs no GPU. Returns
    (hit: bool array over probe, abi.KeysetInfo); raises KeysetError with
    the engine's status (e.g. OBX_NOT_SUPPORTED for a forced bitmap past
    the span cap)."""
    import numpy as np
    k, p = _i64(keys), _i64(probe)
    hit = np.zeros(p.size, dtype=np.uint8)
    info = abi.KeysetInfo()
    rc = lib().obx_gpu_keyset_host_model(
        k.ctypes.data_as(C.c_void_p), k.size, kind,
        p.ctypes.data_as(C.c_void_p), p.size,
        hit.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc != 0:
        raise KeysetError("obx_gpu_keyset_host_model", rc)
    return hit.astype(bool), info


class KeymapError(RuntimeError):
    """A key-map or join-scan verb failed; .rc is the engine's status."""

    def __init__(self, what, rc):
        super().__init__(f"{what} failed: {rc}")
        self.rc = rc


def _payload_args(payloads, spec, n):
    """(uint8 array of n * len datum bytes, abi.ColSchema) of a payload
    column. spec = (obj_type, scale, precision, len); payloads is an integer
    array (the low len bytes of each value are the datum) or an (n, len)
    uint8 array of datum bytes."""
    import numpy as np
    cs = abi.ColSchema(*spec)
    p = np.asarray(payloads)
    if p.dtype == np.uint8 and p.ndim == 2:
        raw = np.ascontiguousarray(p)
        assert raw.shape == (n, cs.len)
    else:
        raw = np.ascontiguousarray(
            _i64(p).view(np.uint8).reshape(-1, 8)[:, :cs.len])
        assert raw.shape[0] == n
    return raw, cs


def keymap_host_model(keys, payloads, spec, probe=(), kind=0):
    """TEST INFRASTRUCTURE: build a key map in host memory with the inline
    functions the device runs and probe it. Needs no GPU. Returns (hit: bool
    array over probe, payload: uint64 array, widened, 0 where not hit,
    abi.KeymapInfo); raises KeymapError with the engine's status."""
    import numpy as np
    k, p = _i64(keys), _i64(probe)
    raw, cs = _payload_args(payloads, spec, k.size)
    hit = np.zeros(p.size, dtype=np.uint8)
    pay = np.zeros(p.size, dtype=np.uint64)
    info = abi.KeymapInfo()
    rc = lib().obx_gpu_keymap_host_model(
        k.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p), k.size,
        C.byref(cs), kind, p.ctypes.data_as(C.c_void_p), p.size,
        hit.ctypes.data_as(C.c_void_p), pay.ctypes.data_as(C.c_void_p),
        C.byref(info))
    if rc != 0:
        raise KeymapError("obx_gpu_keymap_host_model", rc)
    return hit.astype(bool), pay, info


class GroupCapError(RuntimeError):
    """obx_gpu_set_max_groups refused the cap; .rc is the engine's status."""

    def __init__(self, what, rc):
        super().__init__(f"{what} failed: {rc}")
        self.rc = rc


def group_hash_host_model(keys, max_groups, in_flight=0, n_aggs=2):
    """TEST INFRASTRUCTURE: run the sized group table in host memory with
    the inline sizing and find-or-insert functions the device runs: uint64
    keys inserted in order, the stop word looked at every in_flight keys.
    Needs no GPU. Returns a dict: rc (0 or OBX_BUF_NOT_ENOUGH), slots, live
    (keys in the table), max_probe (longest probe sequence, in slots looked
    at), found (input keys a lookup finds afterwards), bytes (of the table at
    n_aggs aggregates). Raises GroupCapError for a cap out of range."""
    import numpy as np
    k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
    out = [C.c_uint64(0) for _ in range(5)]
    rc = lib().obx_gpu_group_hash_host_model(
        k.ctypes.data_as(C.c_void_p), k.size, max_groups, in_flight, n_aggs,
        *[C.byref(o) for o in out])
    if rc not in (0, abi.OBX_BUF_NOT_ENOUGH):
        raise GroupCapError("obx_gpu_group_hash_host_model", rc)
    return dict(rc=rc, slots=out[0].value, live=out[1].value,
                max_probe=out[2].value, found=out[3].value,
                bytes=out[4].value)


class GpuEngine:
    def __init__(self, device=0):
        self._lib = lib()
        self._ctx = C.c_void_p()
        rc = self._lib.obx_gpu_open(device, C.byref(self._ctx))
        if rc == OBX_NO_GPU:
            raise EngineUnavailable("no HIP device visible (product path "
                                    "refuses to run without a GPU)")
        if rc != 0:
            raise RuntimeError(f"obx_gpu_open failed: {rc}")

    def close(self):
        if self._ctx:
            self._lib.obx_gpu_close(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, bs):
        h = self._lib.obx_gpu_load_blocks(self._ctx, C.byref(bs))
        if h < 0:
            raise RuntimeError(f"obx_gpu_load_blocks failed: {h}")
        return h

    def load_cs(self, cs_blocks, schema):
        """GPU-native CS load: device kernels decode the CS streams into
        the engine's scan layout (ObCSMicroBlockTransformer position)."""
        from . import cs as _cs
        bs, keep = _cs.make_blockset(cs_blocks, schema)
        h = self._lib.obx_gpu_load_cs_blocks(self._ctx, C.byref(bs))
        if h < 0:
            raise RuntimeError(f"obx_gpu_load_cs_blocks failed: {h}")
        return h

    def free(self, handle):
        self._lib.obx_gpu_free_blocks(self._ctx, handle)

    # ---- key sets (a join's build keys pushed into the scan) -------------
    def keyset_create(self, keys, kind=0):
        """Device key set of int64 keys (duplicates allowed, may be empty);
        kind 0 auto, 1 hash, 2 bitmap. Returns the set id an
        abi.OP_IN_SET leaf names (dict(col=c, op=OP_IN_SET, set=sid))."""
        k = _i64(keys)
        sid = self._lib.obx_gpu_keyset_create(
            self._ctx, k.ctypes.data_as(C.c_void_p), k.size, kind)
        if sid < 0:
            raise KeysetError("obx_gpu_keyset_create", sid)
        return sid

    def keyset_from_proj(self, handle, proj_idx, kind=0):
        """Key set of projected position proj_idx of the handle's last
        scan_project result, built on the device; NULL rows are skipped and
        the result stays fetchable."""
        sid = self._lib.obx_gpu_keyset_from_proj(self._ctx, handle, proj_idx,
                                                 kind)
        if sid < 0:
            raise KeysetError("obx_gpu_keyset_from_proj", sid)
        return sid

    def keyset_free(self, sid):
        rc = self._lib.obx_gpu_keyset_free(self._ctx, sid)
        if rc != 0:
            raise KeysetError("obx_gpu_keyset_free", rc)

    def keyset_info(self, sid):
        info = abi.KeysetInfo()
        rc = self._lib.obx_gpu_keyset_info(self._ctx, sid, C.byref(info))
        if rc != 0:
            raise KeysetError("obx_gpu_keyset_info", rc)
        return info

    # ---- key maps (a join's build side with one payload column) ----------
    def keymap_create(self, keys, payloads, spec, kind=0):
        """Device key map from distinct int64 keys to one payload datum each
        (see _payload_args for payloads / spec); kind 0 auto, 1 hash,
        2 dense. Returns the map id a scan_join_agg names."""
        k = _i64(keys)
        raw, cs = _payload_args(payloads, spec, k.size)
        mid = self._lib.obx_gpu_keymap_create(
            self._ctx, k.ctypes.data_as(C.c_void_p),
            raw.ctypes.data_as(C.c_void_p), k.size, C.byref(cs), kind)
        if mid < 0:
            raise KeymapError("obx_gpu_keymap_create", mid)
        return mid

    def keymap_from_proj(self, handle, key_idx, payload_idx, kind=0):
        """Key map from projected position key_idx to position payload_idx
        of the handle's last scan_project result, built on the device; rows
        with a NULL key are skipped."""
        mid = self._lib.obx_gpu_keymap_from_proj(self._ctx, handle, key_idx,
                                                 payload_idx, kind)
        if mid < 0:
            raise KeymapError("obx_gpu_keymap_from_proj", mid)
        return mid

    def keymap_free(self, mid):
        rc = self._lib.obx_gpu_keymap_free(self._ctx, mid)
        if rc != 0:
            raise KeymapError("obx_gpu_keymap_free", rc)

    def keymap_info(self, mid):
        info = abi.KeymapInfo()
        rc = self._lib.obx_gpu_keymap_info(self._ctx, mid, C.byref(info))
        if rc != 0:
            raise KeymapError("obx_gpu_keymap_info", rc)
        return info

    def _scan_join_agg(self, handle, filter_desc, map_id, probe_col,
                       agg_desc):
        res = abi.AggResult()
        join = abi.JoinDesc(map_id, probe_col, 0)
        rc = self._lib.obx_gpu_scan_join_agg(
            self._ctx, handle,
            C.byref(filter_desc) if filter_desc is not None else None,
            C.byref(join),
            C.byref(agg_desc) if agg_desc is not None else None,
            C.byref(res))
        return rc, res

    def scan_join_agg(self, handle, filter_desc, map_id, probe_col, agg_desc):
        """scan_filter_agg over the inner join of the table with key map
        map_id on probe_col; abi.COL_JOINED names the map's payload in
        agg_desc. Raises KeymapError (with .rc) on any failure."""
        rc, res = self._scan_join_agg(handle, filter_desc, map_id, probe_col,
                                      agg_desc)
        if rc != 0:
            raise KeymapError("obx_gpu_scan_join_agg", rc)
        return res

    def scan_join_agg_paged(self, handle, filter_desc, map_id, probe_col,
                            agg_desc):
        """The same allowing > OBX_MAX_GROUPS groups: (AggResult, the full
        sorted row list fetched through obx_gpu_agg_fetch)."""
        rc, res = self._scan_join_agg(handle, filter_desc, map_id, probe_col,
                                      agg_desc)
        if rc not in (0, abi.OBX_BUF_NOT_ENOUGH):
            raise KeymapError("obx_gpu_scan_join_agg", rc)
        return res, self.agg_fetch_all(handle)

    def filter(self, handle, filter_desc, want_row_ids=False):
        rc = self._lib.obx_gpu_filter(self._ctx, handle,
                                      C.byref(filter_desc),
                                      1 if want_row_ids else 0)
        if rc != 0:
            raise RuntimeError(f"obx_gpu_filter failed: {rc}")
        return self._lib.obx_gpu_last_survivors(self._ctx, handle)

    def fetch_bitmap(self, handle):
        import numpy as np
        rows = self._lib.obx_gpu_total_rows(self._ctx, handle)
        out = np.zeros((rows + 7) // 8, dtype=np.uint8)
        rc = self._lib.obx_gpu_fetch_bitmap(self._ctx, handle,
                                            out.ctypes.data_as(C.c_void_p),
                                            out.nbytes)
        if rc != 0:
            raise RuntimeError(f"fetch_bitmap failed: {rc}")
        return out

    def fetch_row_ids(self, handle):
        import numpy as np
        rows = self._lib.obx_gpu_total_rows(self._ctx, handle)
        out = np.zeros(rows, dtype=np.int32)
        n = C.c_uint64(0)
        rc = self._lib.obx_gpu_fetch_row_ids(self._ctx, handle,
                                             out.ctypes.data_as(C.c_void_p),
                                             rows, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"fetch_row_ids failed: {rc}")
        return out, int(n.value)

    def fetch_blk_counts(self, handle, n_blocks):
        import numpy as np
        out = np.zeros(n_blocks, dtype=np.uint32)
        rc = self._lib.obx_gpu_fetch_blk_counts(
            self._ctx, handle, out.ctypes.data_as(C.c_void_p), n_blocks)
        if rc != 0:
            raise RuntimeError(f"fetch_blk_counts failed: {rc}")
        return out

    def decode(self, handle, cols):
        arr = (C.c_uint16 * len(cols))(*cols)
        rc = self._lib.obx_gpu_decode(self._ctx, handle, arr, len(cols))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_decode failed: {rc}")

    def fetch_col(self, handle, col, datum_len):
        import numpy as np
        rows = self._lib.obx_gpu_total_rows(self._ctx, handle)
        out = np.zeros(rows * datum_len, dtype=np.uint8)
        rc = self._lib.obx_gpu_fetch_col(self._ctx, handle, col,
                                         out.ctypes.data_as(C.c_void_p),
                                         out.nbytes)
        if rc != 0:
            raise RuntimeError(f"fetch_col failed: {rc}")
        return out

    def scan_project(self, handle, filter_desc, cols, want_row_nos=False):
        """Filter, then decode only the survivors of `cols` (a list of
        column indices, repeats allowed) into dense device vectors in table
        order. filter_desc None = every row. Returns the survivor count;
        fetch_proj / fetch_proj_row_nos page the result out."""
        arr = (C.c_uint16 * len(cols))(*cols)
        n = C.c_uint64(0)
        rc = self._lib.obx_gpu_scan_project(
            self._ctx, handle,
            C.byref(filter_desc) if filter_desc is not None else None,
            arr, len(cols), 1 if want_row_nos else 0, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_scan_project failed: {rc}")
        return int(n.value)

    def _proj_window(self, handle, proj_idx, start, count):
        """rows of [start, start+count) the last scan_project holds"""
        n = C.c_uint64(0)
        rc = self._lib.obx_gpu_fetch_proj(
            self._ctx, handle, proj_idx, start,
            count if count is not None else 2**63, None, 0, None, 0,
            C.byref(n))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_fetch_proj failed: {rc}")
        return int(n.value)

    def fetch_proj(self, handle, proj_idx, datum_len, start=0, count=None):
        """Window [start, start+count) (count None = to the end) of
        projected position proj_idx -> (uint8 array of n*datum_len datum
        bytes, uint8 array of ceil(n/8) null-bitmap bytes: bit i, LSB-first,
        is row start+i, 1 = NULL). NULL rows' datum bytes are zero."""
        import numpy as np
        n = self._proj_window(handle, proj_idx, start, count)
        out = np.zeros(n * datum_len, dtype=np.uint8)
        nulls = np.zeros((n + 7) // 8, dtype=np.uint8)
        got = C.c_uint64(0)
        rc = self._lib.obx_gpu_fetch_proj(
            self._ctx, handle, proj_idx, start, n,
            out.ctypes.data_as(C.c_void_p), out.nbytes,
            nulls.ctypes.data_as(C.c_void_p), nulls.nbytes, C.byref(got))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_fetch_proj failed: {rc}")
        assert got.value == n
        return out, nulls

    def fetch_proj_row_nos(self, handle, start=0, count=None):
        """Table-global row numbers (uint64) of the same window; needs
        scan_project(..., want_row_nos=True)."""
        import numpy as np
        n = C.c_uint64(0)
        rc = self._lib.obx_gpu_fetch_proj_row_nos(
            self._ctx, handle, start, count if count is not None else 2**63,
            None, 0, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_fetch_proj_row_nos failed: {rc}")
        out = np.zeros(n.value, dtype=np.uint64)
        rc = self._lib.obx_gpu_fetch_proj_row_nos(
            self._ctx, handle, start, n.value,
            out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_fetch_proj_row_nos failed: {rc}")
        return out

    def last_proj_stage_ms(self):
        """(filter, block-offset scan, gather) device ms of the last
        scan_project; their sum is last_kernel_ms()."""
        return tuple(float(self._lib.obx_gpu_last_proj_stage_ms(self._ctx, s))
                     for s in range(3))

    def scan_filter_agg(self, handle, filter_desc, agg_desc):
        res = abi.AggResult()
        rc = self._lib.obx_gpu_scan_filter_agg(
            self._ctx, handle,
            C.byref(filter_desc) if filter_desc is not None else None,
            C.byref(agg_desc) if agg_desc is not None else None,
            C.byref(res))
        if rc != 0:
            raise RuntimeError(f"obx_gpu_scan_filter_agg failed: {rc}")
        return res

    def scan_filter_agg_paged(self, handle, filter_desc, agg_desc):
        """Scan allowing > OBX_MAX_GROUPS groups: returns
        (AggResult, [GroupRow...]) with the FULL sorted row list fetched
        through the pagination surface (obx_gpu_agg_fetch)."""
        res = abi.AggResult()
        rc = self._lib.obx_gpu_scan_filter_agg(
            self._ctx, handle,
            C.byref(filter_desc) if filter_desc is not None else None,
            C.byref(agg_desc) if agg_desc is not None else None,
            C.byref(res))
        if rc not in (0, abi.OBX_BUF_NOT_ENOUGH):
            raise RuntimeError(f"obx_gpu_scan_filter_agg failed: {rc}")
        return res, self.agg_fetch_all(handle)

    def agg_fetch_all(self, handle, page=256):
        rows, start = [], 0
        buf = (abi.GroupRow * page)()
        n_out = C.c_uint32()
        total = C.c_uint64()
        while True:
            rc = self._lib.obx_gpu_agg_fetch(self._ctx, handle, start, page,
                                             buf, C.byref(n_out),
                                             C.byref(total))
            if rc != 0:
                raise RuntimeError(f"obx_gpu_agg_fetch failed: {rc}")
            for i in range(n_out.value):
                rows.append(abi.GroupRow.from_buffer_copy(buf[i]))
            start += n_out.value
            if start >= total.value or n_out.value == 0:
                break
        return rows

    # ---- the cap on a scan's distinct groups ------------------------------
    def set_max_groups(self, max_groups):
        """Grant scans of this engine up to max_groups distinct groups
        (default and minimum abi.GROUP_CAP_DEFAULT, at most
        abi.GROUP_CAP_MAX). Raises GroupCapError (with .rc) otherwise."""
        rc = self._lib.obx_gpu_set_max_groups(self._ctx, max_groups)
        if rc != 0:
            raise GroupCapError("obx_gpu_set_max_groups", rc)

    def max_groups(self):
        return int(self._lib.obx_gpu_max_groups(self._ctx))

    def last_group_slots(self):
        """Slots of the sized group table the last aggregate scan ran on;
        0 when it did not need one."""
        return int(self._lib.obx_gpu_last_group_slots(self._ctx))

    def last_group_ms(self):
        """Device ms of the last scan's sized-table kernel (0 = none ran)."""
        return float(self._lib.obx_gpu_last_group_ms(self._ctx))

    def last_kernel_ms(self):
        return float(self._lib.obx_gpu_last_kernel_ms(self._ctx))

    def last_jit(self):
        """True if the last scan ran the hipRTC plan-specialized kernel."""
        return bool(self._lib.obx_gpu_last_jit(self._ctx))

    def last_joint(self):
        """Joint-table form of the last scan's specialized kernel: 0 none,
        1 weights only, 2 one axis with the row count packed into the cell,
        3 two axes (a table under 2 KB) with the row count packed in."""
        return int(self._lib.obx_gpu_last_joint(self._ctx))

    def last_prep_ms(self):
        """Device time of the last query's prep (plan upload + per-block
        filter lowering) — per-operator monitoring, SURVEY §5."""
        return float(self._lib.obx_gpu_last_prep_ms(self._ctx))

    def total_bytes(self, handle):
        return int(self._lib.obx_gpu_total_bytes(self._ctx, handle))

    def total_rows(self, handle):
        return int(self._lib.obx_gpu_total_rows(self._ctx, handle))
