"""ctypes binding of libzkt_plonk_hip.so (the C-ABI declared in include/zkt_plonk.h)."""
from __future__ import annotations

import ctypes
import os
import re
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZKT_LIB_PATH: load another build of the same C-ABI (the host-side sanitizer build of tests/test_host_sanitize.py)
_LIB = os.environ.get("ZKT_LIB_PATH") or os.path.join(_HERE, "libzkt_plonk_hip.so")
_HEADER = os.path.join(_HERE, "..", "include", "zkt_plonk.h")

MSM_BASES_MAX = 1 << 22   # ZKT_MSM_BASES_MAX: most points zkt_msm_g1_bases takes
G1_DECOMPRESS_MAX = 1 << 22              # ZKT_G1_DECOMPRESS_MAX: most points one zkt_g1_decompress takes
VERIFY_BATCH_DEV_MAX = MSM_BASES_MAX // 24   # ZKT_VERIFY_BATCH_DEV_MAX: most proofs one zkt_verify_batch_dev takes
KZG_BATCH_MAX = 32        # ZKT_KZG_BATCH_MAX: most polynomials one zkt_kzg_commit_batch / zkt_kzg_open takes
CURVE_BN254 = 0
CURVE_BLS12_381 = 1
_CURVES = {"bn254": 0, "bls12_381": 1, "bls12-381": 1, 0: 0, 1: 1}

_lib = None


class ZktError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("zkt error %d: %s" % (code, msg))
        self.code = code


def curve_id(curve) -> int:
    return _CURVES[curve]


def lib_path() -> str:
    return _LIB


def declared_symbols():
    """Every function the public header declares (used by the CPU test that checks the exports)."""
    text = open(_HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zkt_[a-z0-9_]+)\s*\(", text)))


def _share_torch_hip_runtime():
    """PyTorch's wheel carries its own libamdhip64.  Two HIP runtimes in one process do not share the device: whichever
    initialises second finds no GPU.  When torch is installed, its copy is mapped first (by path, without importing
    torch), so that this library and torch resolve to the same runtime whatever the import order."""
    import importlib.util
    if os.environ.get("ZKT_SYSTEM_ROCM"):       # a process that will never load torch (tests of the torch-free transport)
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Loads the HIP library.  Raises loudly when it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.environ.get("ZKT_LIB_PATH"):
            _share_torch_hip_runtime()
        if not os.path.exists(_LIB):
            raise ImportError(
                "libzkt_plonk_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'`; the HIP extension is mandatory, there is no CPU fallback." % _LIB)
        L = ctypes.CDLL(_LIB)
        vp, u64p, u32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        L.zkt_version.restype = ctypes.c_char_p
        L.zkt_last_error.restype = ctypes.c_char_p
        L.zkt_last_error.argtypes = [vp]
        L.zkt_ctx_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.zkt_ctx_destroy.argtypes = [vp]
        L.zkt_ctx_destroy.restype = None
        L.zkt_ctx_set_stream.argtypes = [vp, vp]
        L.zkt_ctx_synchronize.argtypes = [vp]
        L.zkt_profile_enable.argtypes = [vp, ctypes.c_int]
        L.zkt_profile_get.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
        L.zkt_dev_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.zkt_dev_free.argtypes = [vp, vp]
        L.zkt_dev_upload.argtypes = [vp, vp, vp, ctypes.c_size_t]
        L.zkt_dev_download.argtypes = [vp, vp, vp, ctypes.c_size_t]
        L.zkt_ntt.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64p, ctypes.c_size_t, u64p]
        L.zkt_ntt_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
        L.zkt_debug_ntt_batch.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp),
                                          ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(vp)]
        L.zkt_debug_ntt_split.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.zkt_domain_group_gen.argtypes = [vp, ctypes.c_int, u64p]
        L.zkt_debug_params.argtypes = [vp, ctypes.c_int, u32p, ctypes.c_size_t]
        L.zkt_debug_fr_mul.argtypes = [vp, u64p, u64p, ctypes.c_size_t, u64p]
        L.zkt_debug_quotient.argtypes = [vp, u64p, ctypes.POINTER(ctypes.c_void_p), u64p, u64p, ctypes.c_size_t, u64p]
        ip = ctypes.POINTER(ctypes.c_int)
        L.zkt_debug_fx_layout.argtypes = [ctypes.c_int, ctypes.c_int, ip, ip, ip]
        L.zkt_host_fx_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p, ctypes.c_size_t, u32p]
        L.zkt_debug_fx_op.argtypes = [vp, ctypes.c_int, ctypes.c_int, u32p, ctypes.c_size_t, u32p]
        L.zkt_host_xyzz_op.argtypes = [ctypes.c_int, ctypes.c_int, u32p, ctypes.c_size_t, u32p]
        L.zkt_debug_xyzz_op.argtypes = [vp, ctypes.c_int, u32p, ctypes.c_size_t, u32p]
        _bind_optional(L)
        _bind_prover(L)
        _bind_witness(L)
        _lib = L
    return _lib


def _bind_optional(L):
    vp, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
    ip = ctypes.POINTER(ctypes.c_int)
    if hasattr(L, "zkt_srs_load"):
        L.zkt_srs_load.argtypes = [vp, u64p, ctypes.c_size_t]
        L.zkt_srs_load_dev.argtypes = [vp, vp, ctypes.c_size_t]
        L.zkt_srs_generate.argtypes = [vp, u64p, ctypes.c_size_t]
        L.zkt_srs_download.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t, u64p]
        L.zkt_msm_g1.argtypes = [vp, u64p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, u64p, ip]
        L.zkt_msm_g1_dev.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, vp]
        L.zkt_msm_enqueue_dev.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
        L.zkt_msm_info.argtypes = [vp, ip, ip, ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(L, "zkt_msm_g1_bases"):
        L.zkt_msm_g1_bases.argtypes = [vp, u64p, u64p, ctypes.c_size_t, ctypes.c_int, u64p, ip]
        L.zkt_msm_g1_bases_dev.argtypes = [vp, vp, vp, ctypes.c_size_t, ctypes.c_int, u64p, ip]
        L.zkt_msm_bases_info.argtypes = [vp, ctypes.c_size_t, ctypes.c_int, ip, ip]
    if hasattr(L, "zkt_g1_decompress"):
        L.zkt_g1_decompress.argtypes = [vp, vp, ctypes.c_size_t, u64p, vp]
        L.zkt_g1_decompress_dev.argtypes = [vp, vp, ctypes.c_size_t, vp, vp]
        vi, tp = ctypes.POINTER(VerifyInputs), ctypes.POINTER(vp)
        L.zkt_verify_batch_prepare_dev.argtypes = [vp, vi, tp, ctypes.c_size_t, u64p, u64p, u64p, ip, u64p]
        L.zkt_verify_batch_dev.argtypes = [vp, vi, tp, ctypes.c_size_t, u64p, u64p, ip]
    if hasattr(L, "zkt_verify_batch_locate"):
        vi, tp = ctypes.POINTER(VerifyInputs), ctypes.POINTER(vp)
        u8p, szp = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_size_t)
        L.zkt_verify_batch_locate.argtypes = [vp, vi, tp, ctypes.c_size_t, u64p, u64p, ip, u8p, szp, szp]
        L.zkt_debug_verify_batch_tree.argtypes = [vp, vi, tp, ctypes.c_size_t, u64p, u64p, u64p, ip, u64p]
        L.zkt_debug_verify_locate_host.argtypes = [ctypes.c_int, vi, tp, ctypes.c_size_t, u64p, u64p, ip, u8p, szp, szp,
                                                   u64p, ip, u64p]
    if hasattr(L, "zkt_srs_check"):
        u8p = ctypes.POINTER(ctypes.c_uint8)
        L.zkt_g1_check.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, u8p]
        L.zkt_debug_g1_check_host.argtypes = [ctypes.c_int, u64p, ctypes.c_size_t, u8p]
        L.zkt_srs_check.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, u64p, u64p, u8p, u8p, ctypes.POINTER(SrsReport)]
        L.zkt_debug_srs_check_chunk.argtypes = [vp, ctypes.c_size_t]
        L.zkt_debug_srs_check_finish_host.argtypes = [ctypes.c_int, u64p, ctypes.c_int, u64p, u64p, ctypes.c_uint64, u64p, u64p,
                                                      u64p, ip]
    if hasattr(L, "zkt_kzg_commit_batch"):
        pp, szp = ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)
        L.zkt_kzg_commit_batch.argtypes = [vp, pp, szp, ctypes.c_int, ctypes.c_int, u64p, ip]
        L.zkt_kzg_commit_batch_dev.argtypes = [vp, pp, szp, ctypes.c_int, ctypes.c_int, u64p, ip]
        L.zkt_kzg_open.argtypes = [vp, pp, szp, ctypes.c_int, u64p, u64p, u64p, ip, u64p]
        L.zkt_kzg_open_dev.argtypes = [vp, pp, szp, ctypes.c_int, u64p, u64p, u64p, ip, u64p]


SRS_CHECK_MAX = (1 << 24) + 1   # ZKT_SRS_CHECK_MAX: most points one zkt_srs_check takes


class SrsReport(ctypes.Structure):
    """zkt_srs_report (include/zkt_plonk.h), field for field."""
    _fields_ = [("count", ctypes.c_uint64), ("n_bad", ctypes.c_uint64), ("first_bad", ctypes.c_uint64),
                ("by_status", ctypes.c_uint64 * 6), ("first_bad_status", ctypes.c_int), ("points_ok", ctypes.c_int),
                ("structure_checked", ctypes.c_int), ("structure_ok", ctypes.c_int), ("ok", ctypes.c_int),
                ("sum_xy_mont", ctypes.c_uint64 * 12), ("sum_is_infinity", ctypes.c_int)]


class SrsCheck:
    """What zkt_srs_check found: the report's fields as plain values; `sum` = (S as (2*fq_limbs,) Montgomery limbs,
    is_infinity) when the structure was checked, else None; `status` the per-point bytes when they were asked for."""

    def __init__(self, r: SrsReport, fq_limbs: int, status=None):
        self.count, self.n_bad, self.first_bad = int(r.count), int(r.n_bad), int(r.first_bad)
        self.by_status = [int(v) for v in r.by_status]
        self.first_bad_status = int(r.first_bad_status)
        self.points_ok, self.structure_checked = bool(r.points_ok), bool(r.structure_checked)
        self.structure_ok, self.ok = bool(r.structure_ok), bool(r.ok)
        self.sum = ((np.array(list(r.sum_xy_mont)[:2 * fq_limbs], dtype=np.uint64), bool(r.sum_is_infinity))
                    if r.structure_checked else None)
        self.status = status

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return ("SrsCheck(ok=%s, count=%d, n_bad=%d, first_bad=%d status %d, structure_checked=%s, structure_ok=%s)"
                % (self.ok, self.count, self.n_bad, self.first_bad, self.first_bad_status, self.structure_checked, self.structure_ok))


def _seed32(seed) -> bytes:
    seed = seed.to_bytes(32, "little") if isinstance(seed, int) else bytes(seed)
    if len(seed) != 32:
        raise ValueError("srs_check: the seed is 32 bytes")
    return seed


def debug_live_allocations():
    """zkt_debug_live_allocations: (count, bytes) of the device allocations the library holds now, over all contexts."""
    L = lib()
    L.zkt_debug_live_allocations.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    count, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = L.zkt_debug_live_allocations(ctypes.byref(count), ctypes.byref(nbytes))
    if rc:
        raise ZktError(rc, "zkt_debug_live_allocations")
    return count.value, nbytes.value


def debug_g1_check_host(curve, points) -> np.ndarray:
    """zkt_debug_g1_check_host: the per-point rules of zkt_g1_check on the host (no device) -> status (n,) uint8."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
    status = np.zeros(pts.shape[0], dtype=np.uint8)
    rc = L.zkt_debug_g1_check_host(cid, u64p(pts) if pts.size else None, pts.shape[0],
                                   status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc:
        raise ZktError(rc, "zkt_debug_g1_check_host")
    return status


def debug_srs_check_finish_host(curve, S, S_inf: bool, P0, Plast, count: int, rho: int, h_g2, beta_h_g2) -> bool:
    """zkt_debug_srs_check_finish_host: the host's end of zkt_srs_check's structure test (no device).  S, P0, Plast:
    (2*fq_limbs,) Montgomery limbs; rho: the challenge as an integer below r -> structure_ok."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    arr = lambda a, n: np.ascontiguousarray(a, dtype=np.uint64).reshape(n)
    S, P0, Plast = arr(S, words), arr(P0, words), arr(Plast, words)
    h, bh = arr(h_g2, 2 * words), arr(beta_h_g2, 2 * words)
    r4 = np.array([(int(rho) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    ok = ctypes.c_int(0)
    rc = L.zkt_debug_srs_check_finish_host(cid, u64p(S), int(bool(S_inf)), u64p(P0), u64p(Plast), count, u64p(r4), u64p(h),
                                           u64p(bh), ctypes.byref(ok))
    if rc:
        raise ZktError(rc, "zkt_debug_srs_check_finish_host")
    return bool(ok.value)


class MerklePathArgs(ctypes.Structure):
    """zkt_merkle_path_args (include/zkt_plonk.h), field for field."""
    _fields_ = [("batch", ctypes.c_size_t), ("height", ctypes.c_int), ("d_variables", ctypes.c_void_p),
                ("n_vars", ctypes.c_size_t), ("d_leaf_var", ctypes.c_void_p), ("d_bit_vars", ctypes.c_void_p),
                ("d_sibling_vars", ctypes.c_void_p), ("d_path_base", ctypes.c_void_p), ("path_base0", ctypes.c_size_t),
                ("d_out_roots", ctypes.c_void_p)]


ALL_GATHER_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_int, ctypes.c_void_p)


ALL_GATHER_ASYNC_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class CommVtable(ctypes.Structure):
    """zkt_comm_vtable (include/zkt_plonk.h): the caller's all-gather for a proof sharded across GPUs; all_gather_async
    (optional) is its stream-ordered form for device buffers."""
    _fields_ = [("user", ctypes.c_void_p), ("rank", ctypes.c_int), ("world", ctypes.c_int),
                ("device_buffers", ctypes.c_int), ("all_gather", ALL_GATHER_CB), ("all_gather_async", ALL_GATHER_ASYNC_CB)]


def shard_range(total: int, rank: int, world: int):
    lo, hi = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L = lib()
    L.zkt_shard_range.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t),
                                  ctypes.POINTER(ctypes.c_size_t)]
    if L.zkt_shard_range(total, rank, world, ctypes.byref(lo), ctypes.byref(hi)):
        raise ValueError("zkt_shard_range(%d, %d, %d)" % (total, rank, world))
    return lo.value, hi.value


def comm_selftest(vt: CommVtable, send: bytes) -> bytes:
    """Gathers `send` from every rank through the vtable (host buffers): plumbing check, no GPU needed."""
    L = lib()
    L.zkt_comm_selftest.argtypes = [ctypes.POINTER(CommVtable), ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    recv = ctypes.create_string_buffer(len(send) * vt.world)
    rc = L.zkt_comm_selftest(ctypes.byref(vt), send, recv, len(send))
    if rc:
        raise ZktError(rc, "zkt_comm_selftest")
    return recv.raw


def keyfile_committer_key(path: str, curve, max_powers: int = 0) -> np.ndarray:
    """--ck file of the reference CLI -> powers_of_g as (count, 2*fq_limbs) Montgomery limbs (host only)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    L.zkt_keyfile_committer_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_size_t)]
    n = ctypes.c_size_t(0)
    rc = L.zkt_keyfile_committer_key(path.encode(), cid, max_powers, None, ctypes.byref(n))
    if rc:
        raise ZktError(rc, "zkt_keyfile_committer_key(%s)" % path)
    out = np.zeros((n.value, words), dtype=np.uint64)
    rc = L.zkt_keyfile_committer_key(path.encode(), cid, max_powers, u64p(out) if out.size else None, ctypes.byref(n))
    if rc:
        raise ZktError(rc, "zkt_keyfile_committer_key(%s)" % path)
    return out


def keyfile_prover_key(path: str, curve):
    """--pk file -> the ten coefficient arrays ((len_k, 4) Montgomery limbs) in zkt_circuit_load order (host only)."""
    L = lib()
    cid = curve_id(curve)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_keyfile_prover_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(P64), ctypes.POINTER(ctypes.c_size_t)]
    lens = (ctypes.c_size_t * 10)()
    rc = L.zkt_keyfile_prover_key(path.encode(), cid, None, lens)
    if rc:
        raise ZktError(rc, "zkt_keyfile_prover_key(%s)" % path)
    arrs = [np.zeros((max(lens[k], 1), 4), dtype=np.uint64) for k in range(10)]
    ptrs = (P64 * 10)(*[u64p(a) for a in arrs])
    rc = L.zkt_keyfile_prover_key(path.encode(), cid, ptrs, lens)
    if rc:
        raise ZktError(rc, "zkt_keyfile_prover_key(%s)" % path)
    return [a[:lens[k]] for k, a in enumerate(arrs)]


def keyfile_extended_prover_key(path: str, curve, which: int = -1):
    """--epk file -> the seventeen vector lengths, and vector `which` as (len, 4) Montgomery limbs (host only, streamed)."""
    L = lib()
    cid = curve_id(curve)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_keyfile_extended_prover_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, P64, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_size_t)]
    lens = (ctypes.c_size_t * 17)()
    rc = L.zkt_keyfile_extended_prover_key(path.encode(), cid, -1, None, 0, lens)
    if rc:
        raise ZktError(rc, "zkt_keyfile_extended_prover_key(%s)" % path)
    if which < 0:
        return list(lens), None
    out = np.zeros((max(lens[which], 1), 4), dtype=np.uint64)
    rc = L.zkt_keyfile_extended_prover_key(path.encode(), cid, which, u64p(out), lens[which], lens)
    if rc:
        raise ZktError(rc, "zkt_keyfile_extended_prover_key(%s, %d)" % (path, which))
    return list(lens), out[:lens[which]]


def keyfile_verifier_key(path: str, curve):
    """--vk file -> (n, pi_roots (k, 4), commitments (10, 2*fq_limbs), is_infinity (10,)); Montgomery limbs (host only)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_keyfile_verifier_key.argtypes = [ctypes.c_char_p, ctypes.c_int, P64, P64, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t), P64, ctypes.POINTER(ctypes.c_int)]
    n, k = ctypes.c_uint64(0), ctypes.c_size_t(0)
    rc = L.zkt_keyfile_verifier_key(path.encode(), cid, ctypes.byref(n), None, 0, ctypes.byref(k), None, None)
    if rc:
        raise ZktError(rc, "zkt_keyfile_verifier_key(%s)" % path)
    roots = np.zeros((max(k.value, 1), 4), dtype=np.uint64)
    commits = np.zeros((10, words), dtype=np.uint64)
    inf = (ctypes.c_int * 10)()
    rc = L.zkt_keyfile_verifier_key(path.encode(), cid, ctypes.byref(n), u64p(roots), roots.shape[0], ctypes.byref(k),
                                    u64p(commits), inf)
    if rc:
        raise ZktError(rc, "zkt_keyfile_verifier_key(%s)" % path)
    return n.value, roots[:k.value], commits, np.array([bool(x) for x in inf])


def keyfile_last_error() -> str:
    """zkt_keyfile_last_error: this thread's last writer failure (the text names the path), "" after a success."""
    L = lib()
    L.zkt_keyfile_last_error.restype = ctypes.c_char_p
    return L.zkt_keyfile_last_error().decode()


def _writer_check(rc: int, what: str):
    if rc:
        raise ZktError(rc, keyfile_last_error() or what)


def notes_write_file(path: str, curve, leaf_indices, identifiers, amounts, secrets):
    """zkt_notes_write_file: the reference CLI's --notes file from leaf indices, identifiers (k, 4), amounts and secrets (k, 4),
    scalars in Montgomery words (host only)."""
    L = lib()
    P64 = ctypes.POINTER(ctypes.c_uint64)
    li = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
    am = np.ascontiguousarray(amounts, dtype=np.uint64).reshape(-1)
    idn = np.ascontiguousarray(identifiers, dtype=np.uint64).reshape(-1, 4)
    sec = np.ascontiguousarray(secrets, dtype=np.uint64).reshape(-1, 4)
    k = li.shape[0]
    assert am.shape[0] == k and idn.shape[0] == k and sec.shape[0] == k
    L.zkt_notes_write_file.argtypes = [ctypes.c_char_p, ctypes.c_int, P64, P64, P64, P64, ctypes.c_size_t]
    p = lambda a: u64p(a) if a.size else None
    _writer_check(L.zkt_notes_write_file(path.encode(), curve_id(curve), p(li), p(idn), p(am), p(sec), k), "zkt_notes_write_file(%s)" % path)


def notes_read_file(path: str, curve):
    """zkt_notes_read_file, both calls -> (leaf_indices (k,), identifiers (k, 4), amounts (k,), secrets (k, 4))."""
    L = lib()
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_notes_read_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t, P64, P64, P64, P64, ctypes.POINTER(ctypes.c_size_t)]
    k = ctypes.c_size_t(0)
    _writer_check(L.zkt_notes_read_file(path.encode(), curve_id(curve), 0, None, None, None, None, ctypes.byref(k)), "zkt_notes_read_file(%s)" % path)
    n = max(k.value, 1)
    li, am = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    idn, sec = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    _writer_check(L.zkt_notes_read_file(path.encode(), curve_id(curve), n, u64p(li), u64p(idn), u64p(am), u64p(sec), ctypes.byref(k)),
                  "zkt_notes_read_file(%s)" % path)
    return li[:k.value], idn[:k.value], am[:k.value], sec[:k.value]


class TreeFileReport(ctypes.Structure):
    """zkt_tree_file_report"""
    _fields_ = [("entries", ctypes.c_uint64), ("mismatches", ctypes.c_uint64), ("first_layer", ctypes.c_int), ("first_idx", ctypes.c_uint64),
                ("root_matches", ctypes.c_int)]


def keyfile_write_committer_key(path: str, curve, powers):
    """zkt_keyfile_write_committer_key: (count, 2*fq_limbs) Montgomery limbs -> the --ck file; an all-zero point is the
    identity (host only)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    pts = np.ascontiguousarray(powers, dtype=np.uint64).reshape(-1, words)
    L.zkt_keyfile_write_committer_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]
    _writer_check(L.zkt_keyfile_write_committer_key(path.encode(), cid, u64p(pts) if pts.size else None, pts.shape[0]),
                  "zkt_keyfile_write_committer_key(%s)" % path)


def keyfile_write_prover_key(path: str, curve, polys):
    """zkt_keyfile_write_prover_key: ten (len_k, 4) coefficient arrays in zkt_circuit_load order -> the --pk file (host only)."""
    L = lib()
    cid = curve_id(curve)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    arrs = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4) for a in polys]
    assert len(arrs) == 10
    ptrs = (P64 * 10)(*[u64p(a) if a.size else P64() for a in arrs])
    lens = (ctypes.c_size_t * 10)(*[a.shape[0] for a in arrs])
    L.zkt_keyfile_write_prover_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(P64), ctypes.POINTER(ctypes.c_size_t)]
    _writer_check(L.zkt_keyfile_write_prover_key(path.encode(), cid, ptrs, lens), "zkt_keyfile_write_prover_key(%s)" % path)


def keyfile_write_verifier_key(path: str, curve, n: int, pi_roots, commitments, is_infinity=None, n_pi: int = None):
    """zkt_keyfile_write_verifier_key: n, pi_roots (k, 4), commitments (10, 2*fq_limbs), is_infinity (10,) or None -> the
    --vk file (host only).  n_pi overrides the number of roots announced (pi_roots None: a NULL pointer)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    P64 = ctypes.POINTER(ctypes.c_uint64)
    roots = None if pi_roots is None else np.ascontiguousarray(pi_roots, dtype=np.uint64).reshape(-1, 4)
    k = (0 if roots is None else roots.shape[0]) if n_pi is None else n_pi
    com = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(10, words)
    inf = None if is_infinity is None else (ctypes.c_int * 10)(*[int(bool(x)) for x in is_infinity])
    L.zkt_keyfile_write_verifier_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64, P64, ctypes.c_size_t, P64,
                                                 ctypes.POINTER(ctypes.c_int)]
    _writer_check(L.zkt_keyfile_write_verifier_key(path.encode(), cid, n, u64p(roots) if roots is not None and roots.size else None, k,
                                                   u64p(com), inf), "zkt_keyfile_write_verifier_key(%s)" % path)


class VerifyInputs(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("vk_commitments", ctypes.POINTER(ctypes.c_uint64)),
                ("vk_is_infinity", ctypes.POINTER(ctypes.c_int)), ("pi_roots", ctypes.POINTER(ctypes.c_uint64)),
                ("pub_inputs", ctypes.POINTER(ctypes.c_uint64)), ("n_pi", ctypes.c_size_t),
                ("proof", ctypes.c_char_p), ("proof_len", ctypes.c_size_t), ("g", ctypes.POINTER(ctypes.c_uint64))]


def verify_prepare(curve, n: int, vk_commits: np.ndarray, vk_inf, pi_roots: np.ndarray, pub_inputs: np.ndarray, proof: bytes,
                   g_xy: np.ndarray, transcript):
    """proof_system/proof.rs:285-503 without the pairings (zkt_verify_prepare; host only).  Arrays are Montgomery limbs;
    `transcript` is a seeded Transcript.  -> (pairs (4, 2*fq_limbs) = L1, W1, L2, W2; is_infinity (4,))."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    vk_commits = np.ascontiguousarray(vk_commits, dtype=np.uint64).reshape(10, words)
    pi_roots = np.ascontiguousarray(pi_roots, dtype=np.uint64).reshape(-1, 4)
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1, 4)
    assert pi_roots.shape == pub_inputs.shape
    g_xy = np.ascontiguousarray(g_xy, dtype=np.uint64).reshape(words)
    inf = (ctypes.c_int * 10)(*[int(bool(x)) for x in vk_inf])
    null = ctypes.POINTER(ctypes.c_uint64)()
    inp = VerifyInputs(n, u64p(vk_commits), inf, u64p(pi_roots) if pi_roots.size else null,
                       u64p(pub_inputs) if pub_inputs.size else null, pi_roots.shape[0], proof, len(proof), u64p(g_xy))
    out = np.zeros((4, words), dtype=np.uint64)
    oinf = (ctypes.c_int * 4)()
    L.zkt_verify_prepare.argtypes = [ctypes.c_int, ctypes.POINTER(VerifyInputs), ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
    rc = L.zkt_verify_prepare(cid, ctypes.byref(inp), transcript.handle, u64p(out), oinf)
    if rc:
        raise ZktError(rc, "zkt_verify_prepare")
    return out, np.array([bool(x) for x in oinf])


def pairing_product_is_one(curve, g1_points: np.ndarray, g2_points: np.ndarray) -> bool:
    """prod_i e(P_i, Q_i) == 1 on the host (zkt_pairing_product_is_one).  g1: (n, 2*fq_limbs); g2: (n, 4*fq_limbs) =
    x.c0, x.c1, y.c0, y.c1; Montgomery limbs."""
    L = lib()
    cid = curve_id(curve)
    words = 4 if cid == CURVE_BN254 else 6
    g1 = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, 2 * words)
    g2 = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, 4 * words)
    assert g1.shape[0] == g2.shape[0]
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_pairing_product_is_one.argtypes = [ctypes.c_int, P64, P64, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    one = ctypes.c_int(0)
    rc = L.zkt_pairing_product_is_one(cid, u64p(g1) if g1.size else None, u64p(g2) if g2.size else None, g1.shape[0],
                                      ctypes.byref(one))
    if rc:
        raise ZktError(rc, "zkt_pairing_product_is_one")
    return bool(one.value)


def verify(curve, n: int, vk_commits, vk_inf, pi_roots, pub_inputs, proof: bytes, g_xy, h_g2, beta_h_g2, transcript) -> bool:
    """Proof::verify (proof_system/proof.rs:285-503) on the host, pairings included (zkt_verify)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    vk_commits = np.ascontiguousarray(vk_commits, dtype=np.uint64).reshape(10, words)
    pi_roots = np.ascontiguousarray(pi_roots, dtype=np.uint64).reshape(-1, 4)
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1, 4)
    g_xy = np.ascontiguousarray(g_xy, dtype=np.uint64).reshape(words)
    h = np.ascontiguousarray(h_g2, dtype=np.uint64).reshape(2 * words)
    bh = np.ascontiguousarray(beta_h_g2, dtype=np.uint64).reshape(2 * words)
    inf = (ctypes.c_int * 10)(*[int(bool(x)) for x in vk_inf])
    null = ctypes.POINTER(ctypes.c_uint64)()
    inp = VerifyInputs(n, u64p(vk_commits), inf, u64p(pi_roots) if pi_roots.size else null,
                       u64p(pub_inputs) if pub_inputs.size else null, pi_roots.shape[0], proof, len(proof), u64p(g_xy))
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_verify.argtypes = [ctypes.c_int, ctypes.POINTER(VerifyInputs), ctypes.c_void_p, P64, P64, ctypes.POINTER(ctypes.c_int)]
    ok = ctypes.c_int(0)
    rc = L.zkt_verify(cid, ctypes.byref(inp), transcript.handle, u64p(h), u64p(bh), ctypes.byref(ok))
    if rc:
        raise ZktError(rc, "zkt_verify")
    return bool(ok.value)


def _verify_batch_args(cid, items, h_g2, beta_h_g2):
    """The C arrays of a batch of verifier inputs -> (ins, transcripts, count, h, beta_h, keep-alive list)."""
    words = 8 if cid == CURVE_BN254 else 12
    h = np.ascontiguousarray(h_g2, dtype=np.uint64).reshape(2 * words)
    bh = np.ascontiguousarray(beta_h_g2, dtype=np.uint64).reshape(2 * words)
    null = ctypes.POINTER(ctypes.c_uint64)()
    k = len(items)
    ins = (VerifyInputs * max(k, 1))()
    trs = (ctypes.c_void_p * max(k, 1))()
    keep = []
    for i, (n, vk_commits, vk_inf, pi_roots, pub_inputs, proof, g_xy, transcript) in enumerate(items):
        vk_commits = np.ascontiguousarray(vk_commits, dtype=np.uint64).reshape(10, words)
        pi_roots = np.ascontiguousarray(pi_roots, dtype=np.uint64).reshape(-1, 4)
        pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1, 4)
        assert pi_roots.shape == pub_inputs.shape
        g_xy = np.ascontiguousarray(g_xy, dtype=np.uint64).reshape(words)
        inf = (ctypes.c_int * 10)(*[int(bool(x)) for x in vk_inf])
        keep.append((vk_commits, pi_roots, pub_inputs, g_xy, inf, proof, transcript))   # the handle dies with its Transcript
        ins[i] = VerifyInputs(n, u64p(vk_commits), inf, u64p(pi_roots) if pi_roots.size else null,
                              u64p(pub_inputs) if pub_inputs.size else null, pi_roots.shape[0], proof, len(proof), u64p(g_xy))
        trs[i] = transcript.handle
    return ins, trs, k, h, bh, keep


def verify_batch(curve, items, h_g2, beta_h_g2) -> bool:
    """zkt_verify_batch: `items` = [(n, vk_commits, vk_inf, pi_roots, pub_inputs, proof bytes, g_xy, seeded Transcript), ...];
    True iff every proof verifies (one product of two pairings for the whole batch)."""
    L = lib()
    cid = curve_id(curve)
    ins, trs, k, h, bh, keep = _verify_batch_args(cid, items, h_g2, beta_h_g2)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_verify_batch.argtypes = [ctypes.c_int, ctypes.POINTER(VerifyInputs), ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t,
                                   P64, P64, ctypes.POINTER(ctypes.c_int)]
    ok = ctypes.c_int(0)
    rc = L.zkt_verify_batch(cid, ins, trs, k, u64p(h), u64p(bh), ctypes.byref(ok))
    if rc:
        raise ZktError(rc, "zkt_verify_batch")
    return bool(ok.value)


def verify_tree_levels(count: int):
    """The level sizes of the tree zkt_verify_batch_locate builds over `count` proofs, leaves first: count,
    ceil(count / 2), ..., 1."""
    sizes = [int(count)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + 1) // 2)
    return sizes


def debug_verify_locate_host(curve, items, h_g2, beta_h_g2, want_tree: bool = True):
    """zkt_debug_verify_locate_host: zkt_verify_batch_locate run on the host, leaves and levels through the code the
    kernels run (no context, no device).  `items` as verify_batch -> (accepted, bad (count,) bool, n_checks, tree), tree =
    None or (nodes (2, n_nodes, 2*fq_limbs) Montgomery limbs for P's and Q's tree, level by level with the leaves first,
    is_infinity (2, n_nodes) bool, rho (2*count, 4) canonical words)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    ins, trs, k, h, bh, keep = _verify_batch_args(cid, items, h_g2, beta_h_g2)
    n_nodes = sum(verify_tree_levels(max(k, 1)))
    ok, nbad, nchk = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    bad = np.zeros(max(k, 1), dtype=np.uint8)
    nodes = np.zeros((2, n_nodes, words), dtype=np.uint64)
    inf = (ctypes.c_int * (2 * n_nodes))()
    rho = np.zeros((2 * max(k, 1), 4), dtype=np.uint64)
    rc = L.zkt_debug_verify_locate_host(cid, ins, trs, k, u64p(h), u64p(bh), ctypes.byref(ok),
                                        bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(nbad), ctypes.byref(nchk),
                                        u64p(nodes) if want_tree else None, inf if want_tree else None,
                                        u64p(rho) if want_tree else None)
    if rc:
        raise ZktError(rc, "zkt_debug_verify_locate_host")
    assert nbad.value == int(bad.sum())
    tree = (nodes, np.array([bool(x) for x in inf]).reshape(2, n_nodes), rho[:2 * k]) if want_tree else None
    return bool(ok.value), bad[:k].astype(bool), nchk.value, tree


def _verify_terms_call(fn, first, cid, items, rho, forced, route):
    """The arguments and results shared by zkt_debug_verify_terms (first = the context handle) and
    zkt_debug_verify_terms_host (first = the curve id)."""
    words = 8 if cid == CURVE_BN254 else 12
    ins, trs, k, _, _, keep = _verify_batch_args(cid, items, np.zeros(2 * words, dtype=np.uint64), np.zeros(2 * words, dtype=np.uint64))
    P64 = ctypes.POINTER(ctypes.c_uint64)
    fn.argtypes = [ctypes.c_void_p if isinstance(first, ctypes.c_void_p) else ctypes.c_int, ctypes.POINTER(VerifyInputs),
                   ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, P64, P64, ctypes.c_int, P64, P64, P64,
                   ctypes.POINTER(ctypes.c_int)]
    rho_a = None if rho is None else np.ascontiguousarray(rho, dtype=np.uint64).reshape(2 * k, 4)
    forced_a = None if forced is None else np.ascontiguousarray(forced, dtype=np.uint64).reshape(k, 7, 4)
    ch = np.zeros((max(k, 1), 7, 4), dtype=np.uint64)
    r0 = np.zeros((max(k, 1), 4), dtype=np.uint64)
    acc = np.zeros((max(k, 1), 24, 4), dtype=np.uint64)
    status = (ctypes.c_int * max(k, 1))()
    rc = fn(first, ins, trs, k, None if rho_a is None else u64p(rho_a), None if forced_a is None else u64p(forced_a), int(route),
            u64p(ch), u64p(r0), u64p(acc), status)
    return rc, (ch[:k], r0[:k], acc[:k], np.array(list(status)[:k], dtype=np.int64))


def debug_verify_terms_host(curve, items, rho=None, forced=None, route: int = 1):
    """zkt_debug_verify_terms_host: the batch verifier's per-proof term stage on the host, no context and no device.  route 0:
    the host verifier's code; route 1: the code the kernel runs.  `items` as verify_batch; rho: None (all ones) or (2*count, 4)
    canonical words; forced: None or (count, 7, 4) Montgomery words beta gamma delta epsilon alpha xi eta that replace the
    transcript's answers.  -> (challenges (count, 7, 4), r0 (count, 4), sums (count, 24, 4), all Montgomery words, status
    (count,) codes); every Transcript of `items` is left where the route left it."""
    cid = curve_id(curve)
    rc, out = _verify_terms_call(lib().zkt_debug_verify_terms_host, cid, cid, items, rho, forced, route)
    if rc:
        raise ZktError(rc, "zkt_debug_verify_terms_host")
    return out


def debug_verify_terms_transcript(transcript, op: int, label: bytes, data: bytes = b"", bits: int = 0) -> bytes:
    """zkt_debug_verify_terms_transcript: one transcript call on `transcript` (a Transcript) through the code the term
    kernel runs, on the host.  op 0: a message (Merlin) or one item given little-endian (Ethereum); op 1: a commitment,
    data = x || y little-endian; op 2: a challenge of `bits` bits -> its 32 little-endian bytes."""
    L = lib()
    L.zkt_debug_verify_terms_transcript.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                                    ctypes.POINTER(ctypes.c_uint8)]
    out = (ctypes.c_uint8 * 32)()
    rc = L.zkt_debug_verify_terms_transcript(transcript.handle, int(op), label, bytes(data), bits if op == 2 else len(data), out)
    if rc:
        raise ZktError(rc, "zkt_debug_verify_terms_transcript")
    return bytes(out)


class ProveInputs(ctypes.Structure):
    _fields_ = [("a_evals", ctypes.POINTER(ctypes.c_uint64)), ("b_evals", ctypes.POINTER(ctypes.c_uint64)),
                ("c_evals", ctypes.POINTER(ctypes.c_uint64)), ("n_rows", ctypes.c_size_t),
                ("table", ctypes.POINTER(ctypes.c_uint64)), ("table_len", ctypes.c_size_t),
                ("pi_pos", ctypes.POINTER(ctypes.c_size_t)), ("pi_vals", ctypes.POINTER(ctypes.c_uint64)),
                ("n_pi", ctypes.c_size_t), ("blinders", ctypes.POINTER(ctypes.c_uint64)),
                ("wires_on_device", ctypes.c_int),
                ("variables", ctypes.POINTER(ctypes.c_uint64)), ("n_vars", ctypes.c_size_t),
                ("w_l", ctypes.POINTER(ctypes.c_uint32)), ("w_r", ctypes.POINTER(ctypes.c_uint32)),
                ("w_o", ctypes.POINTER(ctypes.c_uint32))]


class PoseidonParamsStruct(ctypes.Structure):
    """zkt_poseidon_params"""
    _fields_ = [("width", ctypes.c_int), ("half_full_rounds", ctypes.c_int), ("partial_rounds", ctypes.c_int),
                ("round_constants", ctypes.POINTER(ctypes.c_uint64)), ("mds", ctypes.POINTER(ctypes.c_uint64)),
                ("domain_tag", ctypes.POINTER(ctypes.c_uint64))]


def poseidon_params_struct(width, half_full, partial, round_constants, mds, domain_tag):
    """-> (zkt_poseidon_params, the arrays it points into); all constants as Montgomery words."""
    rc = np.ascontiguousarray(round_constants, dtype=np.uint64).reshape(-1, 4)
    m = np.ascontiguousarray(mds, dtype=np.uint64).reshape(-1, 4)
    tag = np.ascontiguousarray(domain_tag, dtype=np.uint64).reshape(4)
    assert rc.shape[0] == (2 * half_full + partial) * width and m.shape[0] == width * width
    return PoseidonParamsStruct(width, half_full, partial, u64p(rc), u64p(m), u64p(tag)), (rc, m, tag)


class WithdrawInfo(ctypes.Structure):
    """zkt_withdraw_info"""
    _fields_ = [("inputs", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int), ("log_n_min", ctypes.c_int),
                ("n_gates", ctypes.c_size_t), ("n_vars", ctypes.c_size_t), ("n_hashes", ctypes.c_size_t),
                ("vars_per_hash", ctypes.c_size_t), ("n_pi", ctypes.c_size_t), ("device_bytes", ctypes.c_size_t)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class WithdrawRequest(ctypes.Structure):
    """zkt_withdraw_request"""
    _fields_ = [(k, ctypes.POINTER(ctypes.c_uint64)) for k in ("secrets", "identifiers", "amounts", "leaf_indices", "siblings", "root",
                                                               "new_secret", "new_identifier")] + [("withdraw_amount", ctypes.c_uint64)]


class WithdrawProveArgs(ctypes.Structure):
    """zkt_withdraw_prove_args"""
    _fields_ = [("transcript_kind", ctypes.c_int), ("label", ctypes.c_char_p),
                ("identifiers_set", ctypes.POINTER(ctypes.c_uint64)), ("set_len", ctypes.c_size_t),
                ("blinders", ctypes.POINTER(ctypes.c_uint64)),
                ("verify", ctypes.c_int),
                ("g_xy_mont", ctypes.POINTER(ctypes.c_uint64)), ("h_g2_mont", ctypes.POINTER(ctypes.c_uint64)),
                ("beta_h_g2_mont", ctypes.POINTER(ctypes.c_uint64)),
                ("append", ctypes.c_int),
                ("d_variables", ctypes.c_void_p), ("stride", ctypes.c_size_t), ("slots", ctypes.c_size_t)]


class WithdrawResult(ctypes.Structure):
    """zkt_withdraw_result"""
    _fields_ = [("code", ctypes.c_int), ("bad_paths", ctypes.c_uint32), ("verified", ctypes.c_int), ("new_leaf_index", ctypes.c_uint64)]


def _withdraw_requests(requests):
    """zkt_withdraw_request[] from request dictionaries -> (the array, the numpy arrays it points into)."""
    keep, reqs = [], (WithdrawRequest * max(1, len(requests)))()
    null = ctypes.POINTER(ctypes.c_uint64)()
    for r, q in zip(reqs, requests):
        for k in ("secrets", "identifiers", "amounts", "leaf_indices", "siblings", "root", "new_secret", "new_identifier"):
            if q.get(k) is None:
                setattr(r, k, null)
            else:
                a = np.ascontiguousarray(q[k], dtype=np.uint64).reshape(-1)
                keep.append(a)
                setattr(r, k, u64p(a))
        r.withdraw_amount = int(q["withdraw_amount"])
    return reqs, keep


def _withdraw_row_buffers(n_gates, rows, wires):
    P64, P32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    sel = [np.zeros((n_gates, 4), dtype=np.uint64) for _ in range(6)] if rows else None
    w = [np.zeros(n_gates, dtype=np.uint32) for _ in range(3)] if wires else None
    sp = (P64 * 6)(*[u64p(a) for a in sel]) if rows else None
    wp = (P32 * 3)(*[a.ctypes.data_as(P32) for a in w]) if wires else None
    return sel, w, sp, wp


def debug_withdraw_layout_host(curve, params, inputs: int, height: int, rows: bool = True):
    """zkt_debug_withdraw_layout_host: the withdraw circuit's rows as the host planner expands them (no device).  params:
    (width, half_full, partial, round_constants, mds, domain_tag) in Montgomery words.  -> dict with the info fields and, with
    rows, `selectors` (six (n_gates, 4) arrays: q_m, q_l, q_r, q_o, q_c, q_lookup), `wires` (three uint32 arrays), `pi_pos` and
    `hash_calls` ((n_hashes, 5): first variable, arity, three input variables)."""
    L = lib()
    P64, P32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    L.zkt_debug_withdraw_layout_host.argtypes = [ctypes.c_int, ctypes.POINTER(PoseidonParamsStruct), ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(WithdrawInfo), ctypes.POINTER(P64), ctypes.POINTER(P32),
                                                 ctypes.POINTER(ctypes.c_size_t), P32]
    prm, keep = poseidon_params_struct(*params)
    info = WithdrawInfo()
    rc = L.zkt_debug_withdraw_layout_host(curve_id(curve), ctypes.byref(prm), inputs, height, ctypes.byref(info), None, None, None, None)
    if rc:
        raise ZktError(rc, "zkt_debug_withdraw_layout_host")
    out = info.as_dict()
    if rows:
        sel, w, sp, wp = _withdraw_row_buffers(out["n_gates"], True, True)
        pos = (ctypes.c_size_t * out["n_pi"])()
        calls = np.zeros((out["n_hashes"], 5), dtype=np.uint32)
        rc = L.zkt_debug_withdraw_layout_host(curve_id(curve), ctypes.byref(prm), inputs, height, None, sp, wp, pos,
                                              calls.ctypes.data_as(P32))
        if rc:
            raise ZktError(rc, "zkt_debug_withdraw_layout_host")
        out.update(selectors=sel, wires=w, pi_pos=[int(x) for x in pos], hash_calls=calls)
    return out


class WitnessReport(ctypes.Structure):
    """zkt_witness_report"""
    _fields_ = [("satisfied", ctypes.c_int), ("checked", ctypes.c_int),
                ("n_arithmetic", ctypes.c_uint64), ("first_arithmetic", ctypes.c_uint64), ("residual", ctypes.c_uint64 * 4),
                ("n_lookup", ctypes.c_uint64), ("first_lookup", ctypes.c_uint64),
                ("n_wiring", ctypes.c_uint64), ("first_wiring_row", ctypes.c_uint64), ("first_wiring_column", ctypes.c_int)]


CHECK_WIRING = 1                  # ZKT_CHECK_WIRING
CHECK_NONE = (1 << 64) - 1        # ZKT_CHECK_NONE


class WitnessCheck:
    """What zkt_circuit_check_witness found.  `first_*` are rows (None when the rule has no failure), `residual` the gate
    equation's value at first_arithmetic as (4,) Montgomery uint64 limbs, `first_wiring` a (column, row) pair or None;
    `raw` are the struct's bytes."""

    def __init__(self, r: WitnessReport):
        none = lambda v: None if v == CHECK_NONE else int(v)
        self.satisfied = bool(r.satisfied)
        self.checked = int(r.checked)
        self.n_arithmetic, self.first_arithmetic = int(r.n_arithmetic), none(r.first_arithmetic)
        self.residual = np.array(list(r.residual), dtype=np.uint64)
        self.n_lookup, self.first_lookup = int(r.n_lookup), none(r.first_lookup)
        self.n_wiring = int(r.n_wiring)
        self.first_wiring = None if r.first_wiring_row == CHECK_NONE else (int(r.first_wiring_column), int(r.first_wiring_row))
        self.raw = bytes(r)

    def __bool__(self):
        return self.satisfied

    def __repr__(self):
        return ("WitnessCheck(satisfied=%s, checked=%d, arithmetic=%d first %s, lookup=%d first %s, wiring=%d first %s)"
                % (self.satisfied, self.checked, self.n_arithmetic, self.first_arithmetic, self.n_lookup, self.first_lookup,
                   self.n_wiring, self.first_wiring))


class PreparedInputs:
    """A zkt_prove_inputs struct together with the arrays it points into."""

    def __init__(self, struct, keep):
        self.struct = struct
        self._keep = keep


def _bind_prover(L):
    vp, u64p_, u8p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    L.zkt_transcript_new.restype = vp
    L.zkt_transcript_new.argtypes = [ctypes.c_int, ctypes.c_char_p]
    L.zkt_transcript_free.argtypes = [vp]
    L.zkt_transcript_free.restype = None
    L.zkt_transcript_append_u64.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint64]
    L.zkt_transcript_append_u64.restype = None
    L.zkt_transcript_append_scalars.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    L.zkt_transcript_append_scalars.restype = None
    L.zkt_transcript_append_commitment.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                   ctypes.c_size_t, ctypes.c_int]
    L.zkt_transcript_append_commitment.restype = None
    L.zkt_transcript_challenge_scalar.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, u8p]
    L.zkt_transcript_challenge_scalar.restype = None
    L.zkt_transcript_seed.argtypes = [vp, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    L.zkt_transcript_seed.restype = None
    L.zkt_transcript_append_message.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    L.zkt_transcript_challenge_bytes.argtypes = [vp, ctypes.c_char_p, u8p, ctypes.c_size_t]
    L.zkt_circuit_load.argtypes = [vp, ctypes.c_int, ctypes.POINTER(u64p_), ctypes.POINTER(ctypes.c_size_t)]
    L.zkt_circuit_setup.argtypes = [vp, ctypes.c_int, ctypes.POINTER(u64p_), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
                                    u64p_, ctypes.POINTER(ctypes.c_int)]
    L.zkt_circuit_sigma_dev.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.zkt_circuit_setup_wiring.argtypes = [vp, ctypes.c_int, ctypes.POINTER(u64p_), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
                                           vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, u64p_,
                                           ctypes.POINTER(ctypes.c_int)]
    L.zkt_prove.argtypes = [vp, ctypes.POINTER(ProveInputs), vp, u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.zkt_prove_set_next.argtypes = [vp, ctypes.POINTER(ProveInputs)]
    L.zkt_circuit_check_witness.argtypes = [vp, ctypes.POINTER(ProveInputs), ctypes.c_int, ctypes.POINTER(WitnessReport)]


class WitnessPlanReport(ctypes.Structure):
    """zkt_witness_plan_report"""
    _fields_ = [("n_free", ctypes.c_uint64), ("n_out", ctypes.c_uint64), ("n_right", ctypes.c_uint64), ("n_unused", ctypes.c_uint64),
                ("depth", ctypes.c_uint32), ("max_level_rows", ctypes.c_uint32), ("launches", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("device_bytes", ctypes.c_uint64)]


class WitnessStatus(ctypes.Structure):
    """zkt_witness_status"""
    _fields_ = [("n_unsolvable", ctypes.c_uint64), ("first_unsolvable", ctypes.c_uint64)]


WITNESS_BATCH_MAX = 256           # ZKT_WITNESS_BATCH_MAX
WITNESS_RULE_IS_ZERO = 1          # ZKT_WITNESS_RULE_IS_ZERO


class WitnessBatch(ctypes.Structure):
    """zkt_witness_batch"""
    _fields_ = [("d_variables", ctypes.c_void_p), ("stride", ctypes.c_size_t), ("batch", ctypes.c_size_t), ("n_vars", ctypes.c_size_t),
                ("w_l", ctypes.c_void_p), ("w_r", ctypes.c_void_p), ("w_o", ctypes.c_void_p), ("n_rows", ctypes.c_size_t),
                ("wiring_on_device", ctypes.c_int), ("pi_pos", ctypes.POINTER(ctypes.c_size_t)), ("n_pi", ctypes.c_size_t),
                ("d_pi_vals", ctypes.c_void_p), ("tables", ctypes.POINTER(ctypes.POINTER(ctypes.c_uint64))),
                ("table_lens", ctypes.POINTER(ctypes.c_size_t)), ("n_tables", ctypes.c_size_t)]


def _bind_witness(L):
    """zkt_witness_plan_* / zkt_witness_complete*: a missing symbol is an error here, not a fallback."""
    vp, u64p_, u8p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    u32p, szp, sz = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t
    L.zkt_witness_plan_create.argtypes = [vp, vp, vp, vp, sz, sz, ctypes.c_int, szp, sz, ctypes.POINTER(vp)]
    L.zkt_witness_plan_free.argtypes = [vp, vp]
    L.zkt_witness_plan_free.restype = None
    L.zkt_witness_plan_info.argtypes = [vp, ctypes.POINTER(WitnessPlanReport)]
    L.zkt_witness_plan_kinds.argtypes = [vp, u8p]
    L.zkt_witness_complete_enqueue.argtypes = [vp, vp, vp, sz, sz, vp]
    L.zkt_witness_complete_status.argtypes = [vp, vp, sz, ctypes.POINTER(WitnessStatus)]
    L.zkt_witness_complete.argtypes = [vp, vp, u64p_, sz, sz, u64p_, ctypes.POINTER(WitnessStatus)]
    L.zkt_debug_witness_plan_split.argtypes = [vp, ctypes.c_uint32]
    L.zkt_debug_witness_plan_host.argtypes = [ctypes.c_int, ctypes.POINTER(u64p_), ctypes.POINTER(u32p), sz, sz, szp, sz, u8p, u32p,
                                              u32p]
    L.zkt_witness_plan_create_ex.argtypes = [vp, vp, vp, vp, sz, sz, ctypes.c_int, szp, sz, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.zkt_circuit_check_witness_batch.argtypes = [vp, ctypes.POINTER(WitnessBatch), ctypes.c_int, ctypes.POINTER(WitnessReport)]
    L.zkt_debug_witness_plan_host_ex.argtypes = [ctypes.c_int, ctypes.POINTER(u64p_), ctypes.POINTER(u32p), sz, sz, szp, sz, ctypes.c_uint32,
                                                 u8p, u32p, u32p]


def debug_witness_plan_host(curve, selectors, w_l, w_r, w_o, n_vars: int, pi_pos=(), rules: int = 0):
    """zkt_debug_witness_plan_host: the host planner of the witness completion alone (no device).  selectors: q_m q_l q_r q_o
    q_c as (n_rows, 4) Montgomery words; w_*: n_rows uint32 indices (0xFFFFFFFF = Variable::Zero); pi_pos ascending.
    rules: WITNESS_RULE_IS_ZERO or 0 (non-zero goes through zkt_debug_witness_plan_host_ex).
    -> (kind (n_vars,) uint8: 0 on no wire, 1 free, 2 rule O, 3 rule R, 4 / 5 rule Z's y / z; def_row (n_vars,) uint32,
    0xFFFFFFFF when none; level (n_vars,) uint32)."""
    L = lib()
    sel = [np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 4) for q in selectors]
    w = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (w_l, w_r, w_o)]
    n_rows = len(w[0])
    assert len(sel) == 5 and all(q.shape[0] == n_rows for q in sel) and all(len(x) == n_rows for x in w)
    pi = (ctypes.c_size_t * max(len(pi_pos), 1))(*[int(x) for x in pi_pos])
    P64, P32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    sp = (P64 * 5)(*[q.ctypes.data_as(P64) for q in sel])
    wp = (P32 * 3)(*[x.ctypes.data_as(P32) for x in w])
    kind = np.zeros(max(n_vars, 1), dtype=np.uint8)
    def_row, level = np.zeros(max(n_vars, 1), dtype=np.uint32), np.zeros(max(n_vars, 1), dtype=np.uint32)
    outs = (kind.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), def_row.ctypes.data_as(P32), level.ctypes.data_as(P32))
    if rules:
        rc = L.zkt_debug_witness_plan_host_ex(curve_id(curve), sp, wp, n_rows, n_vars, pi, len(pi_pos), int(rules), *outs)
    else:
        rc = L.zkt_debug_witness_plan_host(curve_id(curve), sp, wp, n_rows, n_vars, pi, len(pi_pos), *outs)
    if rc:
        raise ZktError(rc, "zkt_debug_witness_plan_host")
    return kind[:n_vars], def_row[:n_vars], level[:n_vars]


def g1_sum_host(curve, points) -> tuple:
    """Host sum of affine G1 points ((count, 2*fq_limbs) Montgomery limbs, (0,0) = identity) -> (xy limbs, is_infinity).
    The combine step of an index-range-sharded MSM; needs no GPU context."""
    L = lib()
    cid = CURVE_BN254 if curve in ("bn254", CURVE_BN254) else CURVE_BLS12_381
    limbs = 4 if cid == CURVE_BN254 else 6
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2 * limbs)
    out = np.zeros(2 * limbs, dtype=np.uint64)
    inf = ctypes.c_int(0)
    L.zkt_g1_sum_host.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                  ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
    rc = L.zkt_g1_sum_host(cid, u64p(pts) if pts.size else ctypes.POINTER(ctypes.c_uint64)(), pts.shape[0], u64p(out),
                           ctypes.byref(inf))
    if rc:
        raise ZktError(rc, "zkt_g1_sum_host")
    return out, bool(inf.value)


# ---- raw-limb field / curve routines (test hooks; the record layout is described in include/zkt_plonk.h) ----------
def _header_enum(prefix: str) -> dict:
    text = re.sub(r"/\*.*?\*/", "", open(_HEADER).read(), flags=re.S)
    return {m.group(1)[len(prefix):]: int(m.group(2)) for m in re.finditer(r"\b(%s[A-Z0-9_]+)\s*=\s*(\d+)" % prefix, text)}


def fx_ops() -> dict:
    """zkt_fx_op as {name: value}, e.g. "MUL_INL" -> 20 (read from the public header)."""
    return {k: v for k, v in _header_enum("ZKT_FX_").items() if k != "OP_COUNT"}


def xyzz_ops() -> dict:
    return {k: v for k, v in _header_enum("ZKT_XYZZ_").items() if k != "OP_COUNT"}


def fx_layout(curve, which: int) -> tuple:
    """(L, limb_bits, SH) of the field's limb form (zkt_debug_fx_layout)."""
    vals = [ctypes.c_int(0) for _ in range(3)]
    rc = lib().zkt_debug_fx_layout(curve_id(curve), which, *[ctypes.byref(v) for v in vals])
    if rc:
        raise ZktError(rc, "zkt_debug_fx_layout")
    return tuple(v.value for v in vals)


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _records(records, width: int) -> np.ndarray:
    return np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, width)


def host_fx_op(curve, which: int, op: int, records) -> np.ndarray:
    """zkt_host_fx_op on (n, 4 L) u32 records -> (n, 4 L) results, on the host."""
    L_ = fx_layout(curve, which)[0]
    rec = _records(records, 4 * L_)
    out = np.zeros_like(rec)
    rc = lib().zkt_host_fx_op(curve_id(curve), which, op, _u32p(rec), rec.shape[0], _u32p(out))
    if rc:
        raise ZktError(rc, "zkt_host_fx_op")
    return out


def host_xyzz_op(curve, op: int, records) -> np.ndarray:
    """zkt_host_xyzz_op on (n, 2 (4 L + 1)) u32 records -> (n, 4 L + 1) points, on the host."""
    w = 4 * fx_layout(curve, 1)[0] + 1
    rec = _records(records, 2 * w)
    out = np.zeros((rec.shape[0], w), dtype=np.uint32)
    rc = lib().zkt_host_xyzz_op(curve_id(curve), op, _u32p(rec), rec.shape[0], _u32p(out))
    if rc:
        raise ZktError(rc, "zkt_host_xyzz_op")
    return out


def srs_generate_g2(curve, tau: int):
    """The G2 half of the test SRS (zkt_srs_generate_g2): -> (h, beta_h = tau h), each (4 * fq_limbs,) Montgomery limbs in
    arkworks' Fp2 layout -- SonicKZG10 VerifierKey::h / ::beta_h for zkt_verify."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    t = np.array([(int(tau) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    h = np.zeros(2 * words, dtype=np.uint64)
    bh = np.zeros(2 * words, dtype=np.uint64)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_srs_generate_g2.argtypes = [ctypes.c_int, P64, P64, P64]
    rc = L.zkt_srs_generate_g2(cid, u64p(t), u64p(h), u64p(bh))
    if rc:
        raise ZktError(rc, "zkt_srs_generate_g2")
    return h, bh


def g1_msm_host(curve, points, scalars, montgomery: bool = True) -> tuple:
    """HomomorphicCommitment::multi_scalar_mul (commitment.rs:32-45) on arbitrary points, on the host ->
    (xy limbs, is_infinity)."""
    L = lib()
    cid = curve_id(curve)
    words = 8 if cid == CURVE_BN254 else 12
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    assert pts.shape[0] == sc.shape[0]
    out = np.zeros(words, dtype=np.uint64)
    inf = ctypes.c_int(0)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_g1_msm_host.argtypes = [ctypes.c_int, P64, P64, ctypes.c_size_t, ctypes.c_int, P64, ctypes.POINTER(ctypes.c_int)]
    rc = L.zkt_g1_msm_host(cid, u64p(pts) if pts.size else None, u64p(sc) if sc.size else None, pts.shape[0], int(montgomery),
                           u64p(out), ctypes.byref(inf))
    if rc:
        raise ZktError(rc, "zkt_g1_msm_host")
    return out, bool(inf.value)


def quotient_classes_host(curve, log_n: int, windows, challenges):
    """zkt_debug_quotient_classes_host: the host arithmetic of the quotient on three classes (no device).  windows: (10, 14, 4)
    Montgomery words, the coefficients n - 6 .. n + 7 of a b c z1 z2 t sigma1 sigma2 sigma3 q_lookup; challenges: (3, 4) alpha
    beta delta.  -> (u (6, 4), consts (16, 4): X^n on classes 0..3, the inverse Vandermonde matrix row-major, gamma_3^1..3)."""
    L = lib()
    w = np.ascontiguousarray(windows, dtype=np.uint64).reshape(10, 14, 4)
    ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(3, 4)
    u = np.zeros((6, 4), dtype=np.uint64)
    consts = np.zeros((16, 4), dtype=np.uint64)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    L.zkt_debug_quotient_classes_host.argtypes = [ctypes.c_int, ctypes.c_int, P64, P64, P64, P64]
    rc = L.zkt_debug_quotient_classes_host(curve_id(curve), int(log_n), u64p(w), u64p(ch), u64p(u), u64p(consts))
    if rc:
        raise ZktError(rc, "zkt_debug_quotient_classes_host")
    return u, consts


def wire_elimination(curve, selectors, w_l, w_r, w_o, n_vars: int, pi_pos=(), K: int = 16):
    """zkt_debug_wire_elimination: the host pass behind the wire tables over free variables (no device).  selectors: q_m q_l
    q_r q_o q_c as (n_rows, 4) Montgomery words; w_*: n_rows uint32 indices (0xFFFFFFFF = Variable::Zero).  -> (kind (n_vars,)
    uint8: 0 on no wire, 1 free, 2 defined; free (n_free,) uint32; term_v, term_f (n_terms,) uint32; term_coef (n_terms, 4)
    Montgomery words; kappa (n_vars, 4) Montgomery words)."""
    L = lib()
    sel = [np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 4) for q in selectors]
    w = [np.ascontiguousarray(x, dtype=np.uint32) for x in (w_l, w_r, w_o)]
    n_rows = len(w[0])
    assert len(sel) == 5 and all(q.shape[0] == n_rows for q in sel) and all(len(x) == n_rows for x in w)
    pi = (ctypes.c_size_t * max(len(pi_pos), 1))(*[int(x) for x in pi_pos])
    cap = max(K * n_vars, 1)
    kind = np.zeros(max(n_vars, 1), dtype=np.uint8)
    free = np.zeros(max(n_vars, 1), dtype=np.uint32)
    tv, tf = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    tc = np.zeros((cap, 4), dtype=np.uint64)
    kappa = np.zeros((max(n_vars, 1), 4), dtype=np.uint64)
    n_free, n_terms = ctypes.c_size_t(0), ctypes.c_size_t(0)
    P64, P32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    sp = (P64 * 5)(*[u64p(q) for q in sel])
    L.zkt_debug_wire_elimination.argtypes = [ctypes.c_int, ctypes.POINTER(P64), P32, P32, P32, ctypes.c_size_t, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_uint8), P32, ctypes.POINTER(ctypes.c_size_t), P32, P32, P64,
                                             ctypes.POINTER(ctypes.c_size_t), P64]
    rc = L.zkt_debug_wire_elimination(curve_id(curve), sp, _u32p(w[0]), _u32p(w[1]), _u32p(w[2]), n_rows, n_vars, pi, len(pi_pos),
                                      int(K), kind.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _u32p(free), ctypes.byref(n_free),
                                      _u32p(tv), _u32p(tf), u64p(tc), ctypes.byref(n_terms), u64p(kappa))
    if rc:
        raise ZktError(rc, "zkt_debug_wire_elimination")
    nt = n_terms.value
    return kind[:n_vars], free[:n_free.value].copy(), tv[:nt].copy(), tf[:nt].copy(), tc[:nt].copy(), kappa[:n_vars]


class Transcript:
    """Built-in host transcript (T: TranscriptProtocol): kind 'merlin' (plonk-core/src/transcript.rs:46-109)
    or 'ethereum' (gadgets/src/transcript.rs:8-90).  Scalars / coordinates are canonical integers."""

    def __init__(self, kind: str = "merlin", label: str = "ZKT Plonk", fr_bits: int = 254, fq_bytes: int = 32):
        self._L = lib()
        self._h = ctypes.c_void_p(self._L.zkt_transcript_new(0 if kind == "merlin" else 1, label.encode()))
        self.fr_bits = fr_bits
        self.fq_bytes = fq_bytes

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.zkt_transcript_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def append_u64(self, label: str, v: int):
        self._L.zkt_transcript_append_u64(self._h, label.encode(), v)

    def append_scalar(self, label: str, v: int):
        self._L.zkt_transcript_append_scalars(self._h, label.encode(), int(v).to_bytes(32, "little"), 1, 1)

    def append_scalars(self, label: str, vals):
        vals = list(vals)
        self._L.zkt_transcript_append_scalars(self._h, label.encode(),
                                              b"".join(int(v).to_bytes(32, "little") for v in vals), len(vals), 0)

    def append_commitment(self, label: str, point):
        nb = self.fq_bytes
        if point is None:
            self._L.zkt_transcript_append_commitment(self._h, label.encode(), bytes(nb), bytes(nb), nb, 1)
        else:
            self._L.zkt_transcript_append_commitment(self._h, label.encode(), int(point[0]).to_bytes(nb, "little"),
                                                     int(point[1]).to_bytes(nb, "little"), nb, 0)

    def seed(self, circuit_size: int, points):
        """VerifierKey::seed_transcript (keys/mod.rs:260-275) in one call; points: the ten commitments in ProverKey
        order, affine canonical ints or None (identity)."""
        nb = self.fq_bytes
        buf = b"".join(bytes(2 * nb) if p is None else int(p[0]).to_bytes(nb, "little") + int(p[1]).to_bytes(nb, "little")
                       for p in points)
        inf = bytes(1 if p is None else 0 for p in points)
        self._L.zkt_transcript_seed(self._h, circuit_size, buf, inf, nb)

    def challenge_scalar(self, label: str) -> int:
        out = (ctypes.c_uint8 * 32)()
        self._L.zkt_transcript_challenge_scalar(self._h, label.encode(), self.fr_bits, out)
        return int.from_bytes(bytes(out), "little")

    def append_message(self, label: bytes, msg: bytes):
        assert self._L.zkt_transcript_append_message(self._h, label, msg, len(msg)) == 0

    def challenge_bytes(self, label: bytes, n: int) -> bytes:
        out = (ctypes.c_uint8 * n)()
        assert self._L.zkt_transcript_challenge_bytes(self._h, label, out, n) == 0
        return bytes(out)


def u64p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need a C-contiguous uint64 array"
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


class Context:
    """zkt_ctx wrapper: one per caller thread / proof stream."""

    def __init__(self, curve="bn254", device: int = 0):
        self._L = lib()
        self.curve = curve_id(curve)
        self.fq_limbs = 4 if self.curve == CURVE_BN254 else 6
        h = ctypes.c_void_p()
        rc = self._L.zkt_ctx_create(self.curve, device, ctypes.byref(h))
        if rc:
            raise ZktError(rc, "zkt_ctx_create failed (no GPU? there is no CPU fallback)")
        self._h = h
        self.circuit_log_n = None   # log2 n of the circuit loaded through this wrapper (host buffers of the debug hooks)

    def fork(self) -> "Context":
        """zkt_ctx_fork: a context sharing this one's key / circuit / twiddle tables, with its own stream and work buffers."""
        self._L.zkt_ctx_fork.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        h = ctypes.c_void_p()
        self.check(self._L.zkt_ctx_fork(self._h, ctypes.byref(h)))
        other = Context.__new__(Context)
        other.__dict__.update(self.__dict__)
        other._h = h
        return other

    def close(self):
        if getattr(self, "_h", None):
            self._L.zkt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc:
            raise ZktError(rc, self._L.zkt_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: int):
        self.check(self._L.zkt_ctx_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def synchronize(self):
        self.check(self._L.zkt_ctx_synchronize(self._h))

    def profile_enable(self, on: bool = True):
        self.check(self._L.zkt_profile_enable(self._h, int(on)))

    def profile_get(self, name: str):
        """-> (launch count, total milliseconds) measured with HIP events on the context's stream."""
        calls, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
        self.check(self._L.zkt_profile_get(self._h, name.encode(), ctypes.byref(calls), ctypes.byref(ms)))
        return calls.value, ms.value

    # -- one proof across several GPUs --------------------------------------------------------------
    def set_comm(self, comm):
        """Attach a communicator (an object with a `.vt` CommVtable, e.g. parallel.TorchComm) or detach with None.
        Drops whatever SRS / circuit was loaded: keys are laid out for the rank's share."""
        L = self._L
        L.zkt_ctx_set_comm.argtypes = [ctypes.c_void_p, ctypes.POINTER(CommVtable)]
        self._comm = comm                       # keeps the callback alive
        self.check(L.zkt_ctx_set_comm(self._h, ctypes.byref(comm.vt) if comm is not None else None))

    def comm_stats(self):
        """-> (collective calls, bytes sent by this rank) since the communicator was attached."""
        L = self._L
        L.zkt_comm_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.check(L.zkt_comm_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def srs_load_slice(self, pts_slice: np.ndarray, offset: int, total: int):
        pts = np.ascontiguousarray(pts_slice, dtype=np.uint64).reshape(-1, 2 * self.fq_limbs)
        L = self._L
        L.zkt_srs_load_slice.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_size_t,
                                         ctypes.c_size_t]
        self.check(L.zkt_srs_load_slice(self._h, u64p(pts), offset, pts.shape[0], total))

    def srs_generate_slice(self, tau: int, offset: int, count: int, total: int):
        t = np.array([(tau >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        L = self._L
        L.zkt_srs_generate_slice.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                             ctypes.c_size_t, ctypes.c_size_t]
        self.check(L.zkt_srs_generate_slice(self._h, u64p(t), offset, count, total))

    def ntt_class(self, log_n: int, log_big: int, cls: int, arr: np.ndarray) -> np.ndarray:
        """One GPU's share (output indices = cls mod 2^(log_big - log_n)) of the forward coset transform of size
        2^log_big; `arr` may be longer than 2^log_n (folded)."""
        arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
        out = np.empty((1 << log_n, 4), dtype=np.uint64)
        L = self._L
        L.zkt_ntt_class.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                    ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        self.check(L.zkt_ntt_class(self._h, log_n, log_big, cls, u64p(arr), arr.shape[0], u64p(out)))
        return out

    # -- batched Poseidon (witness synthesis) ------------------------------------------------------------
    def poseidon_hash_batch(self, width, half_full, partial, round_constants, mds, domain_tag, inputs, trace=False):
        """plonk-hashing's Poseidon permutation for a batch of inputs ((batch, arity, 4) Montgomery limbs) ->
        hashes (batch, 4) [, states (batch, rounds + 1, width, 4)]."""
        class Params(ctypes.Structure):
            _fields_ = [("width", ctypes.c_int), ("half_full_rounds", ctypes.c_int), ("partial_rounds", ctypes.c_int),
                        ("round_constants", ctypes.POINTER(ctypes.c_uint64)), ("mds", ctypes.POINTER(ctypes.c_uint64)),
                        ("domain_tag", ctypes.POINTER(ctypes.c_uint64))]
        rc = np.ascontiguousarray(round_constants, dtype=np.uint64).reshape(-1, 4)
        m = np.ascontiguousarray(mds, dtype=np.uint64).reshape(width * width, 4)
        tag = np.ascontiguousarray(domain_tag, dtype=np.uint64).reshape(4)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64)
        batch, arity = inp.shape[0], (inp.shape[1] if inp.ndim == 3 else 0)
        rounds = 2 * half_full + partial
        assert rc.shape[0] == rounds * width
        out = np.zeros((batch, 4), dtype=np.uint64)
        st = np.zeros((batch, rounds + 1, width, 4), dtype=np.uint64) if trace else None
        prm = Params(width, half_full, partial, u64p(rc), u64p(m), u64p(tag))
        L = self._L
        L.zkt_poseidon_hash_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.POINTER(ctypes.c_uint64)]
        self.check(L.zkt_poseidon_hash_batch(self._h, ctypes.byref(prm), u64p(inp.reshape(-1, 4)) if inp.size else None, batch,
                                             arity, u64p(out), u64p(st.reshape(-1, 4)) if trace else None))
        return (out, st) if trace else out

    def poseidon_load(self, width, half_full, partial, round_constants, mds, domain_tag) -> int:
        """zkt_poseidon_load: PoseidonConstants resident in HBM -> opaque handle (free with poseidon_free)."""
        class Params(ctypes.Structure):
            _fields_ = [("width", ctypes.c_int), ("half_full_rounds", ctypes.c_int), ("partial_rounds", ctypes.c_int),
                        ("round_constants", ctypes.POINTER(ctypes.c_uint64)), ("mds", ctypes.POINTER(ctypes.c_uint64)),
                        ("domain_tag", ctypes.POINTER(ctypes.c_uint64))]
        rc = np.ascontiguousarray(round_constants, dtype=np.uint64).reshape(-1, 4)
        m = np.ascontiguousarray(mds, dtype=np.uint64).reshape(width * width, 4)
        tag = np.ascontiguousarray(domain_tag, dtype=np.uint64).reshape(4)
        assert rc.shape[0] == (2 * half_full + partial) * width
        prm = Params(width, half_full, partial, u64p(rc), u64p(m), u64p(tag))
        L = self._L
        L.zkt_poseidon_load.argtypes = [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_void_p)]
        h = ctypes.c_void_p()
        self.check(L.zkt_poseidon_load(self._h, ctypes.byref(prm), ctypes.byref(h)))
        return h.value

    def poseidon_free(self, handle: int):
        L = self._L
        L.zkt_poseidon_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.zkt_poseidon_free.restype = None
        L.zkt_poseidon_free(self._h, ctypes.c_void_p(handle))

    def poseidon_hash_batch_dev(self, handle: int, d_inputs: int, batch: int, arity: int, d_hashes: int, d_states: int = 0):
        """zkt_poseidon_hash_batch_dev: device pointers in and out, enqueue only (no allocation, no synchronisation)."""
        L = self._L
        vp = ctypes.c_void_p
        L.zkt_poseidon_hash_batch_dev.argtypes = [vp, vp, vp, ctypes.c_size_t, ctypes.c_int, vp, vp]
        self.check(L.zkt_poseidon_hash_batch_dev(self._h, vp(handle), vp(d_inputs), batch, arity, vp(d_hashes),
                                                 vp(d_states) if d_states else None))

    def poseidon_gadget_vars_per_hash(self, handle: int) -> int:
        L = self._L
        L.zkt_poseidon_gadget_vars_per_hash.argtypes = [ctypes.c_void_p]
        L.zkt_poseidon_gadget_vars_per_hash.restype = ctypes.c_size_t
        return int(L.zkt_poseidon_gadget_vars_per_hash(ctypes.c_void_p(handle)))

    def poseidon_gadget_witness_dev(self, handle: int, batch: int, arity: int, d_variables: int, n_vars: int, d_inputs: int = 0,
                                    d_input_vars: int = 0, d_trace_base: int = 0, trace_base0: int = 0, d_out_hashes: int = 0,
                                    kernel: int = 0, validate_only: bool = False):
        """zkt_poseidon_gadget_witness_dev: the variables PlonkSpecRef's gadget allocates for `batch` independent hashes,
        written in allocation order into the variable map at d_variables (device pointers; enqueue only).
        validate_only: zkt_poseidon_gadget_validate on the same arguments instead (disjoint traces, no input made by the
        same launch; synchronises, launches nothing)."""
        class Args(ctypes.Structure):
            _fields_ = [("batch", ctypes.c_size_t), ("arity", ctypes.c_int), ("d_inputs", ctypes.c_void_p),
                        ("d_input_vars", ctypes.c_void_p), ("d_variables", ctypes.c_void_p), ("n_vars", ctypes.c_size_t),
                        ("d_trace_base", ctypes.c_void_p), ("trace_base0", ctypes.c_size_t), ("d_out_hashes", ctypes.c_void_p),
                        ("kernel", ctypes.c_int)]
        a = Args(batch, arity, d_inputs or None, d_input_vars or None, d_variables or None, n_vars, d_trace_base or None,
                 trace_base0, d_out_hashes or None, kernel)
        L = self._L
        fn = L.zkt_poseidon_gadget_validate if validate_only else L.zkt_poseidon_gadget_witness_dev
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Args)]
        self.check(fn(self._h, ctypes.c_void_p(handle), ctypes.byref(a)))

    def poseidon_gadget_check(self, handle: int):
        """zkt_poseidon_gadget_check: synchronises; raises if a launch skipped a hash (index outside the variable map)."""
        L = self._L
        L.zkt_poseidon_gadget_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.check(L.zkt_poseidon_gadget_check(self._h, ctypes.c_void_p(handle)))

    def merkle_path_vars_per_level(self, handle: int) -> int:
        """zkt_merkle_path_vars_per_level: 6 select variables + the hash's vars_per_hash."""
        L = self._L
        L.zkt_merkle_path_vars_per_level.argtypes = [ctypes.c_void_p]
        L.zkt_merkle_path_vars_per_level.restype = ctypes.c_size_t
        return int(L.zkt_merkle_path_vars_per_level(ctypes.c_void_p(handle)))

    def poseidon_merkle_path_witness_dev(self, handle: int, batch: int, height: int, d_variables: int, n_vars: int,
                                         d_leaf_var: int, d_bit_vars: int, d_sibling_vars: int, d_path_base: int = 0,
                                         path_base0: int = 0, d_out_roots: int = 0, validate_only: bool = False):
        """zkt_poseidon_merkle_path_witness_dev: the variables merkle_proof allocates for `batch` paths of `height` levels
        (per level two conditional_selects and hash_two), one launch, written into the variable map at d_variables (device
        pointers; enqueue only).  validate_only: zkt_poseidon_merkle_path_validate on the same arguments instead (disjoint
        ranges, no input made by the same launch; synchronises, launches nothing)."""
        a = MerklePathArgs(batch, height, d_variables or None, n_vars, d_leaf_var or None, d_bit_vars or None,
                           d_sibling_vars or None, d_path_base or None, path_base0, d_out_roots or None)
        L = self._L
        fn = L.zkt_poseidon_merkle_path_validate if validate_only else L.zkt_poseidon_merkle_path_witness_dev
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(MerklePathArgs)]
        self.check(fn(self._h, ctypes.c_void_p(handle), ctypes.byref(a)))

    # -- the note tree (gadgets/src/merkle_tree.rs) ----------------------------------------------------
    def merkle_tree_create(self, poseidon_handle: int, height: int, capacity: int) -> int:
        """zkt_merkle_tree_create: an empty tree in HBM over a loaded Poseidon (borrowed) -> opaque handle."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_merkle_tree_create.argtypes = [vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(vp)]
        t = vp()
        self.check(L.zkt_merkle_tree_create(self._h, vp(poseidon_handle), height, capacity, ctypes.byref(t)))
        return t.value

    def merkle_tree_free(self, tree: int):
        L = self._L
        L.zkt_merkle_tree_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.zkt_merkle_tree_free.restype = None
        L.zkt_merkle_tree_free(self._h, ctypes.c_void_p(tree))

    def merkle_tree_save_file(self, tree: int, path: str):
        """zkt_merkle_tree_save_file: the tree as the reference CLI's --merkle-tree file."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_merkle_tree_save_file.argtypes = [vp, vp, ctypes.c_char_p]
        self.check(L.zkt_merkle_tree_save_file(self._h, vp(tree), path.encode()))

    def merkle_tree_load_file(self, poseidon: int, height: int, capacity: int, path: str):
        """zkt_merkle_tree_load_file -> (tree handle, report dict): the tree rebuilt from the file's leaves, and how the file's
        other nodes and root compare with it."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_merkle_tree_load_file.argtypes = [vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(vp),
                                                ctypes.POINTER(TreeFileReport)]
        out, rep = vp(0), TreeFileReport()
        self.check(L.zkt_merkle_tree_load_file(self._h, vp(poseidon), height, capacity, path.encode(), ctypes.byref(out), ctypes.byref(rep)))
        return out.value, {"entries": rep.entries, "mismatches": rep.mismatches, "first_layer": rep.first_layer, "first_idx": rep.first_idx,
                           "root_matches": bool(rep.root_matches)}

    def debug_store_chunk(self, nodes: int):
        """zkt_debug_store_chunk: nodes per staging chunk of the tree-file calls on this context (0 = the default)."""
        L = self._L
        L.zkt_debug_store_chunk.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        self.check(L.zkt_debug_store_chunk(self._h, nodes))

    def merkle_tree_append_dev(self, tree: int, d_leaves: int, m: int) -> int:
        """zkt_merkle_tree_append_dev: add_leaf for m device scalars, enqueue only -> index of the first."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_merkle_tree_append_dev.argtypes = [vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        first = ctypes.c_uint64(0)
        self.check(L.zkt_merkle_tree_append_dev(self._h, vp(tree), vp(d_leaves) if d_leaves else None, m, ctypes.byref(first)))
        return first.value

    def merkle_tree_append(self, tree: int, leaves) -> int:
        """zkt_merkle_tree_append: the same with host leaves (m x 4 Montgomery words); synchronises."""
        L, vp = self._L, ctypes.c_void_p
        a = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
        L.zkt_merkle_tree_append.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        first = ctypes.c_uint64(0)
        self.check(L.zkt_merkle_tree_append(self._h, vp(tree), u64p(a) if a.size else None, a.shape[0], ctypes.byref(first)))
        return first.value

    def merkle_tree_root(self, tree: int) -> np.ndarray:
        L, vp = self._L, ctypes.c_void_p
        L.zkt_merkle_tree_root.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint64)]
        out = np.empty(4, dtype=np.uint64)
        self.check(L.zkt_merkle_tree_root(self._h, vp(tree), u64p(out)))
        return out

    def merkle_tree_info(self, tree: int):
        """-> (height, count, capacity)"""
        L = self._L
        L.zkt_merkle_tree_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64)]
        h, n, cap = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = L.zkt_merkle_tree_info(ctypes.c_void_p(tree), ctypes.byref(h), ctypes.byref(n), ctypes.byref(cap))
        if rc:
            raise ZktError(rc, "zkt_merkle_tree_info: null tree")
        return h.value, n.value, cap.value

    def merkle_tree_layer(self, tree: int, layer: int, first: int, n: int) -> np.ndarray:
        """zkt_merkle_tree_layer: the stored nodes (layer, first .. first + n) as n x 4 Montgomery words."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_merkle_tree_layer.argtypes = [vp, vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        out = np.empty((n, 4), dtype=np.uint64)
        self.check(L.zkt_merkle_tree_layer(self._h, vp(tree), layer, first, n, u64p(out) if n else None))
        return out

    def merkle_tree_paths(self, tree: int, indices) -> np.ndarray:
        """zkt_merkle_tree_paths: merkle_path of every index -> k x height x 4 Montgomery words, level 0 first."""
        L, vp = self._L, ctypes.c_void_p
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        L.zkt_merkle_tree_paths.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        out = np.empty((idx.size, self.merkle_tree_info(tree)[0], 4), dtype=np.uint64)
        self.check(L.zkt_merkle_tree_paths(self._h, vp(tree), u64p(idx) if idx.size else None, idx.size, u64p(out) if idx.size else None))
        return out

    def merkle_tree_paths_to_variables_dev(self, tree: int, indices, d_variables: int, n_vars: int, sibling_var0, bit_var0=None):
        """zkt_merkle_tree_paths_to_variables_dev: the siblings (and, with bit_var0, the position bits) of every index
        written into the variable map at d_variables; enqueue only."""
        L, vp, u32p = self._L, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        sib = np.ascontiguousarray(sibling_var0, dtype=np.uint32).reshape(-1)
        bit = None if bit_var0 is None else np.ascontiguousarray(bit_var0, dtype=np.uint32).reshape(-1)
        assert sib.size == idx.size and (bit is None or bit.size == idx.size)
        L.zkt_merkle_tree_paths_to_variables_dev.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, vp,
                                                             ctypes.c_size_t, u32p, u32p]
        self.check(L.zkt_merkle_tree_paths_to_variables_dev(
            self._h, vp(tree), u64p(idx) if idx.size else None, idx.size, vp(d_variables) if d_variables else None, n_vars,
            bit.ctypes.data_as(u32p) if bit is not None else None, sib.ctypes.data_as(u32p)))

    def debug_merkle_tree_split(self, tree: int, wide_min_parents: int):
        """zkt_debug_merkle_tree_split: 1 = every level wide, 2^31 - 1 = every level in the tail, 0 = the policy."""
        L = self._L
        L.zkt_debug_merkle_tree_split.argtypes = [ctypes.c_void_p, ctypes.c_int]
        rc = L.zkt_debug_merkle_tree_split(ctypes.c_void_p(tree), wide_min_parents)
        if rc:
            raise ZktError(rc, "zkt_debug_merkle_tree_split: null tree or negative threshold")

    # -- the withdraw circuit as a component (csrc/withdraw.hip) ----------------------------------------------
    def withdraw_create(self, params, inputs: int, height: int) -> int:
        """zkt_withdraw_create: params = (width, half_full, partial, round_constants, mds, domain_tag) -> opaque handle."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_withdraw_create.argtypes = [vp, ctypes.POINTER(PoseidonParamsStruct), ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        prm, keep = poseidon_params_struct(*params)
        w = vp()
        self.check(L.zkt_withdraw_create(self._h, ctypes.byref(prm), inputs, height, ctypes.byref(w)))
        return w.value

    def withdraw_free(self, w: int):
        L = self._L
        L.zkt_withdraw_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.zkt_withdraw_free.restype = None
        L.zkt_withdraw_free(self._h, ctypes.c_void_p(w))

    def withdraw_poseidon(self, w: int) -> int:
        """zkt_withdraw_poseidon: the handle's own zkt_poseidon, borrowed (bind a MerkleTree to it)."""
        L = self._L
        L.zkt_withdraw_poseidon.argtypes = [ctypes.c_void_p]
        L.zkt_withdraw_poseidon.restype = ctypes.c_void_p
        return L.zkt_withdraw_poseidon(ctypes.c_void_p(w))

    def withdraw_get_info(self, w: int) -> dict:
        L = self._L
        L.zkt_withdraw_get_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(WithdrawInfo)]
        info = WithdrawInfo()
        rc = L.zkt_withdraw_get_info(ctypes.c_void_p(w), ctypes.byref(info))
        if rc:
            raise ZktError(rc, "zkt_withdraw_get_info: null handle")
        return info.as_dict()

    def withdraw_pi_pos(self, w: int):
        L = self._L
        L.zkt_withdraw_pi_pos.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        pos = (ctypes.c_size_t * self.withdraw_get_info(w)["n_pi"])()
        rc = L.zkt_withdraw_pi_pos(ctypes.c_void_p(w), pos)
        if rc:
            raise ZktError(rc, "zkt_withdraw_pi_pos: null handle")
        return [int(x) for x in pos]

    def withdraw_rows(self, w: int, selectors: bool = True, wires: bool = True):
        """zkt_withdraw_rows: the rows regenerated on the device -> (six (n_gates, 4) selector arrays or None, three uint32
        wire arrays or None)."""
        L, vp = self._L, ctypes.c_void_p
        P64, P32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        L.zkt_withdraw_rows.argtypes = [vp, vp, ctypes.POINTER(P64), ctypes.POINTER(P32)]
        sel, wr, sp, wp = _withdraw_row_buffers(self.withdraw_get_info(w)["n_gates"], selectors, wires)
        self.check(L.zkt_withdraw_rows(self._h, vp(w), sp, wp))
        return sel, wr

    def withdraw_setup(self, w: int, log_n: int, table_size: int):
        """zkt_withdraw_setup -> (commitments, is_infinity) as circuit_setup; leaves the circuit loaded."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_withdraw_setup.argtypes = [vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        out = np.zeros((10, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * 10)()
        self.check(L.zkt_withdraw_setup(self._h, vp(w), log_n, table_size, u64p(out), inf))
        self.circuit_log_n = log_n
        return out, np.array([bool(x) for x in inf])

    def withdraw_witness(self, w: int, requests, d_variables: int, stride: int, tree: int = 0, want_pi: bool = True,
                         want_status: bool = True):
        """zkt_withdraw_witness.  requests: dicts with secrets, identifiers (inputs x 4 Montgomery words), amounts,
        leaf_indices (inputs words), siblings ((inputs, height, 4) or None), root ((4,) or None), new_secret, new_identifier
        ((4,)), withdraw_amount.  -> (public inputs (batch, n_pi, 4) or None, [bad_paths] or None); with neither wanted the
        call only enqueues."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_withdraw_witness.argtypes = [vp, vp, ctypes.POINTER(WithdrawRequest), ctypes.c_size_t, vp, vp, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        keep, reqs = [], (WithdrawRequest * max(1, len(requests)))()
        null = ctypes.POINTER(ctypes.c_uint64)()
        for r, q in zip(reqs, requests):
            for k in ("secrets", "identifiers", "amounts", "leaf_indices", "siblings", "root", "new_secret", "new_identifier"):
                if q.get(k) is None:
                    setattr(r, k, null)
                else:
                    a = np.ascontiguousarray(q[k], dtype=np.uint64).reshape(-1)
                    keep.append(a)
                    setattr(r, k, u64p(a))
            r.withdraw_amount = int(q["withdraw_amount"])
        n_pi = self.withdraw_get_info(w)["n_pi"]
        pi = np.zeros((len(requests), n_pi, 4), dtype=np.uint64) if want_pi else None
        st = (ctypes.c_uint32 * max(1, len(requests)))() if want_status else None
        self.check(L.zkt_withdraw_witness(self._h, vp(w), reqs, len(requests), vp(tree) if tree else None, vp(d_variables) if d_variables else None,
                                          stride, u64p(pi) if want_pi else None, st))
        return pi, ([int(x) for x in st[:len(requests)]] if want_status else None)

    def withdraw_prepare(self, w: int, d_variables: int, stride: int, b: int, table, pi_vals, blinders) -> "PreparedInputs":
        """zkt_withdraw_prove_inputs for request b of a map made by withdraw_witness, with the caller's table, public-input
        values (in position order) and blinders."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_withdraw_prove_inputs.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ProveInputs)]
        null = ctypes.POINTER(ctypes.c_uint64)()
        prep = self._prepare((null, null, null), 0, table, self.withdraw_pi_pos(w), pi_vals, blinders, True)
        rc = L.zkt_withdraw_prove_inputs(vp(w), vp(d_variables), stride, b, prep.struct.pi_pos, prep.struct.pi_vals, ctypes.byref(prep.struct))
        if rc:
            raise ZktError(rc, "zkt_withdraw_prove_inputs: null pointer or stride below n_vars")
        return prep

    def withdraw_prove(self, w: int, requests, d_variables: int, stride: int, slots: int, identifiers_set, blinders, tree: int = 0,
                       transcript_kind: str = "merlin", label: str = "ZKT Plonk", verify_key=None, append: bool = False):
        """zkt_withdraw_prove: ProveWithdraw for every request in one call.  requests as withdraw_witness takes them;
        identifiers_set (k, 4) and blinders (batch, 19, 4) Montgomery words; verify_key = (g, h, beta_h) to have each proof
        checked; `slots` maps of `stride` scalars at d_variables.  -> ([proof bytes], public inputs (batch, n_pi, 4),
        [{code, bad_paths, verified, new_leaf_index}]); a proof that was not made is b""."""
        L, vp = self._L, ctypes.c_void_p
        P64 = ctypes.POINTER(ctypes.c_uint64)
        batch = len(requests)
        reqs, keep = _withdraw_requests(requests)
        ids = np.ascontiguousarray(identifiers_set, dtype=np.uint64).reshape(-1, 4)
        bl = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
        assert bl.size == batch * 19 * 4
        vk = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in verify_key] if verify_key is not None else None
        args = WithdrawProveArgs(0 if transcript_kind == "merlin" else 1 if transcript_kind == "ethereum" else int(transcript_kind), label.encode(),
                                 u64p(ids) if ids.size else P64(), ids.shape[0], u64p(bl) if bl.size else P64(), int(vk is not None),
                                 u64p(vk[0]) if vk else P64(), u64p(vk[1]) if vk else P64(), u64p(vk[2]) if vk else P64(), int(bool(append)),
                                 d_variables or None, stride, slots)
        n_pi = self.withdraw_get_info(w)["n_pi"]
        plen = 802 if self.curve == CURVE_BN254 else 1010
        proofs = np.zeros((max(batch, 1), plen), dtype=np.uint8)
        pi = np.zeros((batch, n_pi, 4), dtype=np.uint64)
        res = (WithdrawResult * max(batch, 1))()
        L.zkt_withdraw_prove.argtypes = [vp, vp, ctypes.POINTER(WithdrawRequest), ctypes.c_size_t, vp, ctypes.POINTER(WithdrawProveArgs),
                                         ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t, P64, ctypes.POINTER(WithdrawResult)]
        self.check(L.zkt_withdraw_prove(self._h, vp(w), reqs, batch, vp(tree) if tree else None, ctypes.byref(args),
                                        proofs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), plen, u64p(pi) if pi.size else P64(), res))
        out = [dict(code=r.code, bad_paths=r.bad_paths, verified=bool(r.verified), new_leaf_index=r.new_leaf_index) for r in res[:batch]]
        return [proofs[b].tobytes() if out[b]["code"] == 0 else b"" for b in range(batch)], pi, out

    def note_leaves(self, poseidon_handle: int, d_secrets: int, d_identifiers: int, d_amounts: int, m: int, d_out_leaves: int):
        """zkt_note_leaves: leaf = H(identifier, amount, H(secret)) for m deposits, device pointers; synchronises."""
        L, vp = self._L, ctypes.c_void_p
        L.zkt_note_leaves.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
        self.check(L.zkt_note_leaves(self._h, vp(poseidon_handle), vp(d_secrets) if d_secrets else None, vp(d_identifiers) if d_identifiers else None,
                                     vp(d_amounts) if d_amounts else None, m, vp(d_out_leaves) if d_out_leaves else None))

    # -- witness completion from the free variables (csrc/witness_plan.hip) ---------------------------------
    def witness_plan_create(self, w_l, w_r, w_o, n_vars: int, pi_pos=(), n_rows: int = None, rules: int = 0) -> int:
        """zkt_witness_plan_create over the loaded circuit: w_* are uint32 arrays (host) or device pointers (ints, with
        n_rows given); pi_pos ascending -> opaque plan handle.  rules != 0 (WITNESS_RULE_IS_ZERO) goes through
        zkt_witness_plan_create_ex."""
        vp = ctypes.c_void_p
        on_device = isinstance(w_l, int)
        if on_device:
            ptrs, keep = [vp(x) if x else None for x in (w_l, w_r, w_o)], ()
            assert n_rows is not None
        else:
            keep = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (w_l, w_r, w_o)]
            n_rows = len(keep[0]) if n_rows is None else n_rows
            ptrs = [vp(x.ctypes.data) if x.size else None for x in keep]
        pos = (ctypes.c_size_t * max(1, len(pi_pos)))(*[int(x) for x in pi_pos])
        plan = vp()
        if rules:
            self.check(self._L.zkt_witness_plan_create_ex(self._h, ptrs[0], ptrs[1], ptrs[2], n_rows, n_vars, int(on_device), pos,
                                                          len(pi_pos), int(rules), ctypes.byref(plan)))
        else:
            self.check(self._L.zkt_witness_plan_create(self._h, ptrs[0], ptrs[1], ptrs[2], n_rows, n_vars, int(on_device), pos,
                                                       len(pi_pos), ctypes.byref(plan)))
        return plan.value

    def witness_plan_free(self, plan: int):
        self._L.zkt_witness_plan_free(self._h, ctypes.c_void_p(plan))

    def witness_plan_info(self, plan: int) -> dict:
        """zkt_witness_plan_info -> {n_free, n_out, n_right, n_unused, depth, max_level_rows, launches, n_pairs, device_bytes};
        n_pairs is the struct's `reserved` word, the number of rule-Z pairs (0 for a plan made without the bit)."""
        r = WitnessPlanReport()
        rc = self._L.zkt_witness_plan_info(ctypes.c_void_p(plan), ctypes.byref(r))
        if rc:
            raise ZktError(rc, "zkt_witness_plan_info: null plan")
        return {("n_pairs" if k == "reserved" else k): int(getattr(r, k)) for k, _ in WitnessPlanReport._fields_}

    def witness_plan_kinds(self, plan: int, n_vars: int) -> np.ndarray:
        out = np.zeros(max(n_vars, 1), dtype=np.uint8)
        rc = self._L.zkt_witness_plan_kinds(ctypes.c_void_p(plan), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        if rc:
            raise ZktError(rc, "zkt_witness_plan_kinds: null plan")
        return out[:n_vars]

    def debug_witness_plan_split(self, plan: int, wide_min_rows: int):
        """zkt_debug_witness_plan_split: 0 = the policy."""
        rc = self._L.zkt_debug_witness_plan_split(ctypes.c_void_p(plan), wide_min_rows)
        if rc:
            raise ZktError(rc, "zkt_debug_witness_plan_split: null plan")

    def witness_complete_enqueue(self, plan: int, d_variables: int, stride: int, batch: int = 1, d_out_pi: int = 0):
        """zkt_witness_complete_enqueue: enqueue only."""
        vp = ctypes.c_void_p
        self.check(self._L.zkt_witness_complete_enqueue(self._h, vp(plan), vp(d_variables) if d_variables else None, stride, batch,
                                                    vp(d_out_pi) if d_out_pi else None))

    def witness_complete_status(self, plan: int, batch: int = 1):
        """zkt_witness_complete_status -> [(unsolvable rows, the smallest such row or None)] per witness; synchronises, clears."""
        out = (WitnessStatus * max(batch, 1))()
        self.check(self._L.zkt_witness_complete_status(self._h, ctypes.c_void_p(plan), batch, out))
        return [(int(s.n_unsolvable), None if s.first_unsolvable == CHECK_NONE else int(s.first_unsolvable)) for s in out[:batch]]

    def witness_complete(self, plan: int, variables, n_pi: int, stride: int = None):
        """zkt_witness_complete on a host map of (batch, stride, 4) or (stride, 4) Montgomery words -> (the completed maps
        (batch, stride, 4), public inputs (batch, n_pi, 4), status as witness_complete_status gives it)."""
        v = np.array(variables, dtype=np.uint64, order="C")
        v = v.reshape((1,) + v.shape) if v.ndim == 2 else v
        batch, stride = v.shape[0], (v.shape[1] if stride is None else stride)
        pi = np.zeros((batch, max(n_pi, 1), 4), dtype=np.uint64)
        st = (WitnessStatus * batch)()
        self.check(self._L.zkt_witness_complete(self._h, ctypes.c_void_p(plan), u64p(v) if v.size else None, stride, batch, u64p(pi), st))
        return v, pi[:, :n_pi], [(int(s.n_unsolvable), None if s.first_unsolvable == CHECK_NONE else int(s.first_unsolvable)) for s in st]

    # -- device memory ------------------------------------------------------------------------
    def alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        self.check(self._L.zkt_dev_alloc(self._h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, dptr: int):
        self.check(self._L.zkt_dev_free(self._h, ctypes.c_void_p(dptr)))

    def upload(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self.check(self._L.zkt_dev_upload(self._h, ctypes.c_void_p(dptr), arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes))

    def download(self, dptr: int, shape, dtype=np.uint64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self.check(self._L.zkt_dev_download(self._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dptr), out.nbytes))
        return out

    # -- Domain seam ------------------------------------------------------------------------------
    def ntt(self, log_n: int, arr: np.ndarray, inverse=False, coset=False) -> np.ndarray:
        arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
        out = np.empty((1 << max(log_n, 0), 4), dtype=np.uint64)
        self.check(self._L.zkt_ntt(self._h, log_n, int(inverse), int(coset), u64p(arr), arr.shape[0], u64p(out)))
        return out

    def ntt_dev(self, log_n: int, d_in: int, in_len: int, d_out: int, inverse=False, coset=False):
        self.check(self._L.zkt_ntt_dev(self._h, log_n, int(inverse), int(coset), ctypes.c_void_p(d_in), in_len,
                                       ctypes.c_void_p(d_out)))

    def group_gen(self, log_n: int) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint64)
        self.check(self._L.zkt_domain_group_gen(self._h, log_n, u64p(out)))
        return out

    # -- Commitment seam ----------------------------------------------------------------------------
    def srs_load(self, pts: np.ndarray):
        pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 2 * self.fq_limbs)
        self.check(self._L.zkt_srs_load(self._h, u64p(pts), pts.shape[0]))

    def srs_load_dev(self, d_pts: int, count: int):
        """zkt_srs_load_dev: `count` powers (x || y Montgomery limbs each) already resident in HBM (device pointer)."""
        self.check(self._L.zkt_srs_load_dev(self._h, ctypes.c_void_p(d_pts), count))

    def srs_load_file(self, ck_path: str, max_powers: int = 0):
        """zkt_srs_load from the reference CLI's --ck file (CommitterKey.powers_of_g)."""
        L = self._L
        L.zkt_srs_load_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        self.check(L.zkt_srs_load_file(self._h, ck_path.encode(), max_powers))

    def circuit_load_file(self, pk_path: str, log_n: int):
        """zkt_circuit_load from the reference CLI's --pk file (ProverKey<F>)."""
        L = self._L
        L.zkt_circuit_load_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        self.check(L.zkt_circuit_load_file(self._h, pk_path.encode(), log_n))
        self.circuit_log_n = log_n

    def srs_generate(self, tau: int, count: int):
        t = np.array([(tau >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        self.check(self._L.zkt_srs_generate(self._h, u64p(t), count))

    def srs_download(self, offset: int, count: int) -> np.ndarray:
        out = np.empty((count, 2 * self.fq_limbs), dtype=np.uint64)
        self.check(self._L.zkt_srs_download(self._h, offset, count, u64p(out)))
        return out

    def msm(self, scalars: np.ndarray, base_offset: int = 0, montgomery: bool = True):
        """-> (xy Montgomery limbs (2*fq_limbs,), is_infinity)"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(2 * self.fq_limbs, dtype=np.uint64)
        inf = ctypes.c_int(0)
        self.check(self._L.zkt_msm_g1(self._h, u64p(scalars), scalars.shape[0], base_offset, int(montgomery),
                                      u64p(out), ctypes.byref(inf)))
        return out, bool(inf.value)

    def msm_dev(self, d_scalars: int, n: int, base_offset: int = 0, montgomery: bool = True) -> np.ndarray:
        out = np.zeros(2 * self.fq_limbs, dtype=np.uint64)
        self.check(self._L.zkt_msm_g1_dev(self._h, ctypes.c_void_p(d_scalars), n, base_offset, int(montgomery),
                                          out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def msm_enqueue_dev(self, d_scalars: int, n: int, base_offset: int = 0, montgomery: bool = True):
        self.check(self._L.zkt_msm_enqueue_dev(self._h, ctypes.c_void_p(d_scalars), n, base_offset, int(montgomery)))

    def msm_bases(self, bases: np.ndarray, scalars: np.ndarray, montgomery: bool = True):
        """zkt_msm_g1_bases: sum scalars[i] * bases[i] over the caller's points (no SRS needed) ->
        (xy Montgomery limbs (2*fq_limbs,), is_infinity)"""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 2 * self.fq_limbs)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        if bases.shape[0] != scalars.shape[0]:
            raise ValueError("msm_bases: %d bases, %d scalars" % (bases.shape[0], scalars.shape[0]))
        n = bases.shape[0]
        out = np.zeros(2 * self.fq_limbs, dtype=np.uint64)
        inf = ctypes.c_int(0)
        self.check(self._L.zkt_msm_g1_bases(self._h, u64p(bases) if n else None, u64p(scalars) if n else None, n,
                                            int(montgomery), u64p(out), ctypes.byref(inf)))
        return out, bool(inf.value)

    def msm_bases_dev(self, d_bases: int, d_scalars: int, n: int, montgomery: bool = True):
        """zkt_msm_g1_bases_dev: bases (n x 2*fq_limbs words) and scalars (n x 4 words) already in HBM ->
        (xy Montgomery limbs, is_infinity)"""
        out = np.zeros(2 * self.fq_limbs, dtype=np.uint64)
        inf = ctypes.c_int(0)
        self.check(self._L.zkt_msm_g1_bases_dev(self._h, ctypes.c_void_p(d_bases), ctypes.c_void_p(d_scalars), n,
                                                int(montgomery), u64p(out), ctypes.byref(inf)))
        return out, bool(inf.value)

    # ---- untrusted bytes: checked deserialisation and batch verification on the device ----
    def g1_decompress(self, data):
        """zkt_g1_decompress: `data` = n compressed G1 points (bytes, 32 each on BN254, 48 on BLS12-381) ->
        (points (n, 2*fq_limbs) Montgomery limbs, (0,0) for the identity and refused points; status (n,) uint8)"""
        nb = 8 * self.fq_limbs
        data = bytes(data)
        if len(data) % nb:
            raise ValueError("g1_decompress: %d bytes is not a whole number of %d-byte points" % (len(data), nb))
        n = len(data) // nb
        out = np.zeros((n, 2 * self.fq_limbs), dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint8)
        self.check(self._L.zkt_g1_decompress(self._h, data if n else None, n, u64p(out) if n else None,
                                             status.ctypes.data_as(ctypes.c_void_p) if n else None))
        return out, status

    def g1_decompress_dev(self, d_in: int, n: int, d_out: int, d_status: int):
        """zkt_g1_decompress_dev: n x nb bytes in HBM -> n points and n status bytes in HBM; only enqueues."""
        self.check(self._L.zkt_g1_decompress_dev(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out),
                                                 ctypes.c_void_p(d_status)))

    # ---- an untrusted committer key: per-point validation and the structure test on the device ----
    def _check_points(self, points, n):
        """(pointer, count, on_device, keep) of a host array of points, or of a device pointer with its count n"""
        if isinstance(points, int):
            if n is None:
                raise ValueError("a device pointer needs its point count")
            return ctypes.c_void_p(points), int(n), 1, None
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2 * self.fq_limbs)
        return ctypes.c_void_p(pts.ctypes.data if pts.size else None), pts.shape[0], 0, pts

    def g1_check(self, points, n: int = None) -> np.ndarray:
        """zkt_g1_check: `points` = a (n, 2*fq_limbs) array of (x, y) Montgomery limbs, or a device pointer (int) to n such
        points -> status (n,) uint8, one ZKT_G1_* value per point.  Synchronises the stream."""
        ptr, n, on_dev, keep = self._check_points(points, n)
        status = np.zeros(n, dtype=np.uint8)
        self.check(self._L.zkt_g1_check(self._h, ptr, n, on_dev, status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return status

    def srs_check(self, points, h_g2, beta_h_g2, seed, n: int = None, want_status: bool = False) -> SrsCheck:
        """zkt_srs_check: are `points` (array or device pointer, as g1_check) the powers_of_g of the key whose VerifierKey
        holds h and beta_h?  seed: 32 bytes (or an integer below 2^256) the caller drew at random -> SrsCheck."""
        ptr, n, on_dev, keep = self._check_points(points, n)
        h = np.ascontiguousarray(h_g2, dtype=np.uint64).reshape(4 * self.fq_limbs)
        bh = np.ascontiguousarray(beta_h_g2, dtype=np.uint64).reshape(4 * self.fq_limbs)
        seed = (ctypes.c_uint8 * 32)(*_seed32(seed))
        status = np.zeros(max(n, 1), dtype=np.uint8) if want_status else None
        rep = SrsReport()
        self.check(self._L.zkt_srs_check(self._h, ptr, n, on_dev, u64p(h), u64p(bh), seed,
                                         status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if want_status else None,
                                         ctypes.byref(rep)))
        return SrsCheck(rep, self.fq_limbs, status[:n] if want_status else None)

    def debug_srs_check_chunk(self, max_points: int):
        """zkt_debug_srs_check_chunk: points per chunk of this context's later srs_check calls; 0 restores the default."""
        self.check(self._L.zkt_debug_srs_check_chunk(self._h, max_points))

    def verify_batch_prepare_dev(self, items, h_g2, beta_h_g2, want_rho: bool = True):
        """zkt_verify_batch_prepare_dev: `items` as _lib.verify_batch -> (A, B) as a (2, 2*fq_limbs) array of Montgomery limbs,
        their two infinity flags, and the 2 * len(items) folding coefficients as (m, 4) canonical words (None unless
        want_rho).  The batch is valid iff e(A, h) e(-B, beta h) == 1."""
        ins, trs, k, h, bh, keep = _verify_batch_args(self.curve, items, h_g2, beta_h_g2)
        ab = np.zeros((2, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * 2)()
        rho = np.zeros((2 * max(k, 1), 4), dtype=np.uint64) if want_rho else None
        self.check(self._L.zkt_verify_batch_prepare_dev(self._h, ins, trs, k, u64p(h), u64p(bh), u64p(ab), inf,
                                                        u64p(rho) if want_rho else None))
        return ab, np.array([bool(x) for x in inf]), (rho[:2 * k] if want_rho else None)

    def verify_batch_dev(self, items, h_g2, beta_h_g2) -> bool:
        """zkt_verify_batch_dev: `items` as _lib.verify_batch; True iff every proof verifies.  Decompression and the two
        combinations run on the device, the transcripts and the one pairing product on the host."""
        ins, trs, k, h, bh, keep = _verify_batch_args(self.curve, items, h_g2, beta_h_g2)
        ok = ctypes.c_int(0)
        self.check(self._L.zkt_verify_batch_dev(self._h, ins, trs, k, u64p(h), u64p(bh), ctypes.byref(ok)))
        return bool(ok.value)

    def verify_batch_locate(self, items, h_g2, beta_h_g2):
        """zkt_verify_batch_locate: `items` as _lib.verify_batch -> (accepted, bad, n_checks): whether every proof verifies,
        a (count,) bool array naming the proofs that do not, and the pairing checks made (1 for an accepted batch, at most
        1 + 2 * bad.sum() * ceil(log2(count)) otherwise).  The pairs of a rejected batch and their tree are formed on the
        device, the tree is searched on the host."""
        ins, trs, k, h, bh, keep = _verify_batch_args(self.curve, items, h_g2, beta_h_g2)
        ok, nbad, nchk = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        bad = np.zeros(max(k, 1), dtype=np.uint8)
        self.check(self._L.zkt_verify_batch_locate(self._h, ins, trs, k, u64p(h), u64p(bh), ctypes.byref(ok),
                                                   bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(nbad),
                                                   ctypes.byref(nchk)))
        assert nbad.value == int(bad.sum())
        return bool(ok.value), bad[:k].astype(bool), nchk.value

    def debug_verify_batch_tree(self, items, h_g2, beta_h_g2):
        """zkt_debug_verify_batch_tree: the pairs of every proof and their tree from the device, whatever the verdict ->
        (nodes (2, n_nodes, 2*fq_limbs), is_infinity (2, n_nodes), rho (2*count, 4)) as _lib.debug_verify_locate_host."""
        ins, trs, k, h, bh, keep = _verify_batch_args(self.curve, items, h_g2, beta_h_g2)
        n_nodes = sum(verify_tree_levels(max(k, 1)))
        nodes = np.zeros((2, n_nodes, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * (2 * n_nodes))()
        rho = np.zeros((2 * max(k, 1), 4), dtype=np.uint64)
        self.check(self._L.zkt_debug_verify_batch_tree(self._h, ins, trs, k, u64p(h), u64p(bh), u64p(nodes), inf, u64p(rho)))
        return nodes, np.array([bool(x) for x in inf]).reshape(2, n_nodes), rho[:2 * k]

    def set_verify_terms(self, mode: int = 0):
        """zkt_ctx_set_verify_terms: where the batch verifier runs its transcripts and scalar stage, 0 on the host (the
        default), 1 on the device; results do not depend on it"""
        self._L.zkt_ctx_set_verify_terms.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.check(self._L.zkt_ctx_set_verify_terms(self._h, int(mode)))

    def debug_verify_terms(self, items, rho=None, forced=None, route: int = 2):
        """zkt_debug_verify_terms: the term stage alone, the commitments through the device's decompression; route 0 the
        host code, route 2 the kernel.  Arguments and results as _lib.debug_verify_terms_host."""
        rc, out = _verify_terms_call(self._L.zkt_debug_verify_terms, self._h, self.curve, items, rho, forced, route)
        self.check(rc)
        return out

    def msm_bases_info(self, n: int, montgomery: bool = True):
        """-> dict(window_bits, windows) that zkt_msm_g1_bases uses for n points"""
        c, w = ctypes.c_int(0), ctypes.c_int(0)
        self.check(self._L.zkt_msm_bases_info(self._h, n, int(montgomery), ctypes.byref(c), ctypes.byref(w)))
        return dict(window_bits=c.value, windows=w.value)

    # ---- KZG commitment seam (zkt_kzg_commit_batch / zkt_kzg_open) ----
    def _kzg_polys(self, polys):
        arrs = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a.shape[0] else None for a in arrs])
        return arrs, ptrs, self._kzg_lens([a.shape[0] for a in arrs])

    @staticmethod
    def _kzg_lens(lens):
        return (ctypes.c_size_t * max(len(lens), 1))(*[int(n) for n in lens])

    def _kzg_points(self, out, inf, k):
        W = 2 * self.fq_limbs
        return [(out[j * W:(j + 1) * W].copy(), bool(inf[j])) for j in range(k)]

    def kzg_commit_batch(self, polys, montgomery: bool = True):
        """zkt_kzg_commit_batch: PC::commit of every coefficient vector in `polys` (arrays of (len, 4) u64) in one call ->
        [(xy Montgomery limbs (2*fq_limbs,), is_infinity)] in order"""
        arrs, ptrs, lens = self._kzg_polys(polys)
        k = len(arrs)
        out = np.zeros(max(k, 1) * 2 * self.fq_limbs, dtype=np.uint64)
        inf = (ctypes.c_int * max(k, 1))()
        self.check(self._L.zkt_kzg_commit_batch(self._h, ptrs, lens, k, int(montgomery), u64p(out), inf))
        return self._kzg_points(out, inf, k)

    def kzg_commit_batch_dev(self, d_ptrs, lens, montgomery: bool = True):
        """zkt_kzg_commit_batch_dev: the coefficient vectors already in HBM (device pointers, lengths in elements)"""
        k = len(lens)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[int(d) if d else None for d in d_ptrs])
        out = np.zeros(max(k, 1) * 2 * self.fq_limbs, dtype=np.uint64)
        inf = (ctypes.c_int * max(k, 1))()
        self.check(self._L.zkt_kzg_commit_batch_dev(self._h, ptrs, self._kzg_lens(lens), k, int(montgomery), u64p(out), inf))
        return self._kzg_points(out, inf, k)

    def _kzg_open_call(self, fn, ptrs, lens, k, challenges, z, evals):
        ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4)
        if ch.shape[0] != k:
            raise ValueError("kzg_open: %d polynomials, %d challenges" % (k, ch.shape[0]))
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(4)
        w = np.zeros(2 * self.fq_limbs, dtype=np.uint64)
        inf = ctypes.c_int(0)
        ev = np.zeros((max(k, 1), 4), dtype=np.uint64)
        self.check(fn(self._h, ptrs, lens, k, u64p(ch) if k else None, u64p(zz), u64p(w), ctypes.byref(inf),
                      u64p(ev) if evals else None))
        return (w, bool(inf.value)), (ev[:k].copy() if evals else None)

    def kzg_open(self, polys, challenges, z, evals: bool = True):
        """zkt_kzg_open: w = commit(floor((sum_j challenges[j] polys[j]) / (X - z))), all Montgomery ->
        ((xy, is_infinity), evaluations p_j(z) as a (k, 4) array, or None when evals is False)"""
        arrs, ptrs, lens = self._kzg_polys(polys)
        return self._kzg_open_call(self._L.zkt_kzg_open, ptrs, lens, len(arrs), challenges, z, evals)

    def kzg_open_dev(self, d_ptrs, lens, challenges, z, evals: bool = True):
        """zkt_kzg_open_dev: kzg_open over coefficient vectors already in HBM"""
        k = len(lens)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[int(d) if d else None for d in d_ptrs])
        return self._kzg_open_call(self._L.zkt_kzg_open_dev, ptrs, self._kzg_lens(lens), k, challenges, z, evals)

    def msm_info(self):
        c, w, n = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
        self.check(self._L.zkt_msm_info(self._h, ctypes.byref(c), ctypes.byref(w), ctypes.byref(n)))
        return dict(window_bits=c.value, windows=w.value, srs_count=n.value)

    # -- commitments of evaluation vectors (Lagrange-basis key, include/zkt_plonk.h) ----------------------
    def set_lagrange(self, on: bool = True):
        self._L.zkt_ctx_set_lagrange.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.check(self._L.zkt_ctx_set_lagrange(self._h, int(on)))

    def set_wire_elimination(self, mode: int = 1):
        """zkt_ctx_set_wire_elimination: 0 off, 1 automatic (circuits of 2^17 rows and more), 2 whenever a table can be built"""
        self._L.zkt_ctx_set_wire_elimination.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.check(self._L.zkt_ctx_set_wire_elimination(self._h, int(mode)))

    def lagrange_info(self):
        self._L.zkt_lagrange_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
        lg, nb = ctypes.c_int(0), ctypes.c_size_t(0)
        self.check(self._L.zkt_lagrange_info(self._h, ctypes.byref(lg), ctypes.byref(nb)))
        return dict(log_n=lg.value, bases=nb.value)

    def commit_evals_dev(self, d_evals: int, blinders=None, path: int = 1):
        """PC::commit(poly_from_evals(evals) + blinders): path 0 through the coefficients, 1 through the Lagrange basis.
        -> (xy Montgomery limbs, is_infinity); the domain is the loaded circuit's."""
        self._L.zkt_commit_evals_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                                 ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        k = 0 if blinders is None else int(np.asarray(blinders).reshape(-1, 4).shape[0])
        bl = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4) if k else None
        out = np.zeros(2 * self.fq_limbs, dtype=np.uint64)
        inf = ctypes.c_int(0)
        self.check(self._L.zkt_commit_evals_dev(self._h, ctypes.c_void_p(d_evals), u64p(bl) if k else None, k, int(path),
                                                u64p(out), ctypes.byref(inf)))
        return out, bool(inf.value)

    # -- prover -----------------------------------------------------------------------------------------
    def circuit_load(self, log_n: int, pk_polys):
        """pk_polys: 10 arrays (len_k, 4) in the order q_m q_l q_r q_o q_c sigma1 sigma2 sigma3 q_lookup q_table."""
        arrs = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in pk_polys]
        assert len(arrs) == 10
        ptrs = (ctypes.POINTER(ctypes.c_uint64) * 10)(*[u64p(a) if a.size else ctypes.POINTER(ctypes.c_uint64)() for a in arrs])
        lens = (ctypes.c_size_t * 10)(*[a.shape[0] for a in arrs])
        self.check(self._L.zkt_circuit_load(self._h, log_n, ptrs, lens))
        self.circuit_log_n = log_n

    def circuit_setup(self, log_n: int, evals):
        """proof_system::setup (setup.rs:42-166) on the device.  evals: the 10 evaluation vectors (len_k <= n, 4) in
        ProverKey order, Montgomery limbs.  Leaves the circuit loaded; -> (commitments (10, 2*fq_limbs) Montgomery
        limbs, is_infinity (10,) bool) = the VerifierKey commitments in the same order."""
        arrs = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in evals]
        assert len(arrs) == 10
        ptrs = (ctypes.POINTER(ctypes.c_uint64) * 10)(*[u64p(a) if a.size else ctypes.POINTER(ctypes.c_uint64)() for a in arrs])
        lens = (ctypes.c_size_t * 10)(*[a.shape[0] for a in arrs])
        out = np.zeros((10, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * 10)()
        self.check(self._L.zkt_circuit_setup(self._h, log_n, ptrs, lens, 0, u64p(out), inf))
        self.circuit_log_n = log_n
        return out, np.array([bool(x) for x in inf])

    def circuit_sigma(self, log_n: int, d_w_l: int, d_w_r: int, d_w_o: int, n_rows: int, n_vars: int, d_sigma=None):
        """zkt_circuit_sigma_dev: compute_all_sigma_evals (permutation/mod.rs:103-177) from the wiring resident in HBM
        (three device pointers to n_rows uint32 indices, 0xFFFFFFFF = Variable::Zero).  d_sigma: three device pointers
        of n * 32 bytes that receive sigma1..3; None: -> the three vectors as (n, 4) Montgomery uint64 host arrays."""
        n = 1 << log_n if 0 <= log_n <= 25 else 0
        own = d_sigma is None
        if own:
            d_sigma = [self.alloc(max(n, 1) * 32) for _ in range(3)]
        try:
            ptrs = (ctypes.c_void_p * 3)(*d_sigma)
            self.check(self._L.zkt_circuit_sigma_dev(self._h, log_n, ctypes.c_void_p(d_w_l), ctypes.c_void_p(d_w_r),
                                                     ctypes.c_void_p(d_w_o), n_rows, n_vars, ptrs))
            return [self.download(p, (n, 4)) for p in d_sigma] if own else None
        finally:
            if own:
                for p in d_sigma:
                    self.free(p)

    def circuit_setup_wiring(self, log_n: int, evals, w_l, w_r, w_o, n_vars: int, n_rows: int = None):
        """zkt_circuit_setup_wiring: proof_system::setup from the composer's own data.  evals: the 10 vectors of
        circuit_setup with entries 5, 6, 7 (sigma1..3) None; w_l / w_r / w_o: uint32 index arrays (host), or three
        device pointers (ints) together with n_rows.  -> (commitments, is_infinity) as circuit_setup."""
        assert len(evals) == 10
        arrs = [np.zeros((0, 4), dtype=np.uint64) if p is None else np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4)
                for p in evals]
        ptrs = (ctypes.POINTER(ctypes.c_uint64) * 10)(*[u64p(a) if a.size else ctypes.POINTER(ctypes.c_uint64)() for a in arrs])
        lens = (ctypes.c_size_t * 10)(*[a.shape[0] for a in arrs])
        on_device = isinstance(w_l, int)
        if on_device:
            assert n_rows is not None
            w = [ctypes.c_void_p(p) for p in (w_l, w_r, w_o)]
        else:
            idx = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (w_l, w_r, w_o)]
            assert idx[0].shape == idx[1].shape == idx[2].shape
            n_rows = idx[0].shape[0] if n_rows is None else n_rows
            w = [x.ctypes.data_as(ctypes.c_void_p) if x.size else ctypes.c_void_p() for x in idx]
        out = np.zeros((10, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * 10)()
        self.check(self._L.zkt_circuit_setup_wiring(self._h, log_n, ptrs, lens, 0, w[0], w[1], w[2], n_rows, n_vars,
                                                    int(on_device), u64p(out), inf))
        self.circuit_log_n = log_n
        return out, np.array([bool(x) for x in inf])

    def _prepare(self, wires, n_rows, table, pi_pos, pi_vals, blinders, on_device, variables=None, idx=None, keep=()):
        table = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 4)
        pi_vals = np.ascontiguousarray(pi_vals, dtype=np.uint64).reshape(-1, 4)
        if blinders is None:          # zkt_circuit_check_witness ignores them; zkt_prove refuses a NULL pointer
            blinders = np.zeros((0, 4), dtype=np.uint64)
        else:
            blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(19, 4)
        pos = (ctypes.c_size_t * max(1, len(pi_pos)))(*pi_pos)
        null = ctypes.POINTER(ctypes.c_uint64)()
        null32 = ctypes.POINTER(ctypes.c_uint32)()
        inp = ProveInputs(wires[0], wires[1], wires[2], n_rows, u64p(table) if table.size else null, table.shape[0],
                          pos, u64p(pi_vals) if pi_vals.size else null, len(pi_pos), u64p(blinders) if blinders.size else null, int(on_device),
                          variables[0] if variables else null, variables[1] if variables else 0,
                          idx[0] if idx else null32, idx[1] if idx else null32, idx[2] if idx else null32)
        return PreparedInputs(inp, (table, pi_vals, blinders, pos) + tuple(keep))

    def prepare_dev(self, d_a: int, d_b: int, d_c: int, n_rows: int, table, pi_pos, pi_vals, blinders) -> "PreparedInputs":
        """zkt_prove_inputs for wire vectors already resident in HBM (device pointers), built once and reusable: the
        prefetch of zkt_prove_set_next recognises the next proof by the identity of these pointers."""
        cast = lambda p: ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_uint64))
        return self._prepare((cast(d_a), cast(d_b), cast(d_c)), n_rows, table, pi_pos, pi_vals, blinders, True)

    def prepare_host(self, a, b, c, table, pi_pos, pi_vals, blinders) -> "PreparedInputs":
        """zkt_prove_inputs for wire vectors in host memory ((n_rows, 4) Montgomery uint64 arrays, kept alive here)."""
        a, b, c = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (a, b, c))
        null = ctypes.POINTER(ctypes.c_uint64)()
        return self._prepare(tuple(u64p(x) if x.size else null for x in (a, b, c)), a.shape[0], table, pi_pos, pi_vals,
                             blinders, False, keep=(a, b, c))

    def prepare_vars(self, variables, w_l, w_r, w_o, table, pi_pos, pi_vals, blinders) -> "PreparedInputs":
        """zkt_prove_inputs in the composer's own witness layout (host memory): `variables` (n_vars, 4) Montgomery
        values and three uint32 index vectors (0xFFFFFFFF = Variable::Zero); prove.rs:49-55 runs on the device."""
        variables = np.ascontiguousarray(variables, dtype=np.uint64).reshape(-1, 4)
        idx = [np.ascontiguousarray(w, dtype=np.uint32).reshape(-1) for w in (w_l, w_r, w_o)]
        assert idx[0].shape == idx[1].shape == idx[2].shape
        null = ctypes.POINTER(ctypes.c_uint64)()
        u32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        return self._prepare((null, null, null), idx[0].shape[0], table, pi_pos, pi_vals, blinders, False,
                             variables=(u64p(variables) if variables.size else null, variables.shape[0]),
                             idx=[u32p(x) for x in idx], keep=(variables, idx))

    def prepare_vars_dev(self, d_variables: int, n_vars: int, d_w_l: int, d_w_r: int, d_w_o: int, n_rows: int, table, pi_pos,
                         pi_vals, blinders) -> "PreparedInputs":
        """The composer's witness layout with everything resident in HBM (wires_on_device = 1): `d_variables` may be a
        buffer a device kernel filled, e.g. the states of zkt_poseidon_hash_batch_dev."""
        c64 = lambda p: ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_uint64))
        c32 = lambda p: ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_uint32))
        null = ctypes.POINTER(ctypes.c_uint64)()
        return self._prepare((null, null, null), n_rows, table, pi_pos, pi_vals, blinders, True,
                             variables=(c64(d_variables), n_vars), idx=[c32(d_w_l), c32(d_w_r), c32(d_w_o)])

    def prove_prepared(self, prep: "PreparedInputs", transcript, next_prep: "PreparedInputs" = None) -> bytes:
        """zkt_prove on prepared inputs.  next_prep announces the proof that follows (zkt_prove_set_next): its
        challenge-free rounds 1 and 2 are issued behind this proof's last commitments."""
        self.check(self._L.zkt_prove_set_next(self._h, ctypes.byref(next_prep.struct) if next_prep is not None else None))
        out = (ctypes.c_uint8 * 2048)()
        n = ctypes.c_size_t(0)
        self.check(self._L.zkt_prove(self._h, ctypes.byref(prep.struct), transcript.handle, out, 2048, ctypes.byref(n)))
        return bytes(out[:n.value])

    def check_witness(self, prep: "PreparedInputs", flags: int = 0) -> "WitnessCheck":
        """zkt_circuit_check_witness: check_gate (constraint_system/helper.rs:13-75) over every row of the loaded circuit
        on prepared inputs (any of prepare_host / prepare_dev / prepare_vars / prepare_vars_dev; the blinders are ignored).
        flags = CHECK_WIRING also compares the wiring of a variables-form witness with the key's permutation.  An
        unsatisfied witness is a result, not an error."""
        rep = WitnessReport()
        self.check(self._L.zkt_circuit_check_witness(self._h, ctypes.byref(prep.struct), int(flags), ctypes.byref(rep)))
        return WitnessCheck(rep)

    def witness_batch(self, d_variables: int, stride: int, batch: int, n_vars: int, w_l, w_r, w_o, pi_pos=(), d_pi_vals: int = 0,
                      tables=(), n_rows: int = None) -> "PreparedInputs":
        """A zkt_witness_batch with the arrays it points into: `batch` maps in HBM at d_variables, `stride` scalars apart, one
        wiring (uint32 arrays, or device pointers as ints with n_rows given), d_pi_vals (batch, n_pi) in HBM in the order of
        pi_pos, `tables` a list of 0, 1 or `batch` host tables of (len, 4) Montgomery words."""
        vp = ctypes.c_void_p
        on_device = isinstance(w_l, int)
        if on_device:
            ptrs, keep = [x or None for x in (w_l, w_r, w_o)], []
            assert n_rows is not None
        else:
            keep = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (w_l, w_r, w_o)]
            n_rows = len(keep[0]) if n_rows is None else n_rows
            ptrs = [x.ctypes.data if x.size else None for x in keep]
        pos = (ctypes.c_size_t * max(1, len(pi_pos)))(*[int(x) for x in pi_pos])
        tabs = [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1, 4) for t in tables]
        P64 = ctypes.POINTER(ctypes.c_uint64)
        tp = (P64 * max(1, len(tabs)))(*[u64p(t) if t.size else P64() for t in tabs])
        tl = (ctypes.c_size_t * max(1, len(tabs)))(*[t.shape[0] for t in tabs])
        st = WitnessBatch(d_variables or None, stride, batch, n_vars, ptrs[0], ptrs[1], ptrs[2], n_rows, int(on_device), pos, len(pi_pos),
                          d_pi_vals or None, tp, tl, len(tabs))
        return PreparedInputs(st, (keep, pos, tabs, tp, tl))

    def check_witness_batch(self, wb: "PreparedInputs", flags: int = 0):
        """zkt_circuit_check_witness_batch on a witness_batch(...) -> [WitnessCheck] per witness, each what check_witness
        reports for that witness alone.  Enqueues behind the work on the context's stream, synchronises once."""
        reps = (WitnessReport * max(1, int(wb.struct.batch)))()
        self.check(self._L.zkt_circuit_check_witness_batch(self._h, ctypes.byref(wb.struct), int(flags), reps))
        return [WitnessCheck(r) for r in reps[:wb.struct.batch]]

    def prove_dev(self, d_a: int, d_b: int, d_c: int, n_rows: int, table, pi_pos, pi_vals, blinders, transcript) -> bytes:
        """Same as prove() with the three wire vectors already resident in HBM (device pointers)."""
        return self.prove_prepared(self.prepare_dev(d_a, d_b, d_c, n_rows, table, pi_pos, pi_vals, blinders), transcript)

    def prove(self, a, b, c, table, pi_pos, pi_vals, blinders, transcript) -> bytes:
        """proof_system::prove (prove.rs:59-470); all arrays are (len, 4) Montgomery uint64."""
        return self.prove_prepared(self.prepare_host(a, b, c, table, pi_pos, pi_vals, blinders), transcript)

    def prove_vars(self, variables, w_l, w_r, w_o, table, pi_pos, pi_vals, blinders, transcript) -> bytes:
        """proof_system::prove from the composer's own witness layout (see prepare_vars)."""
        return self.prove_prepared(self.prepare_vars(variables, w_l, w_r, w_o, table, pi_pos, pi_vals, blinders), transcript)

    # -- debug hooks ----------------------------------------------------------------------------------
    def debug_params(self, which: int):
        buf = (ctypes.c_uint32 * 64)()
        n = self._L.zkt_debug_params(self._h, which, buf, 64)
        w = list(buf)
        to_int = lambda l: sum(int(x) << (32 * i) for i, x in enumerate(l))
        return dict(p=to_int(w[0:n]), inv32=int(w[n]), r=to_int(w[n + 1:2 * n + 1]), r2=to_int(w[2 * n + 1:3 * n + 1]))

    def debug_ntt_batch(self, log_n: int, d_in, in_len, d_out, inverse=False, coset=False, nb=None):
        """zkt_debug_ntt_batch: nb transforms of one plan in one launch per pass; device pointers, lengths in elements."""
        nb = len(d_in) if nb is None else nb
        ins, outs = (ctypes.c_void_p * len(d_in))(*d_in), (ctypes.c_void_p * len(d_out))(*d_out)
        lens = (ctypes.c_size_t * len(in_len))(*in_len)
        self.check(self._L.zkt_debug_ntt_batch(self._h, log_n, int(inverse), int(coset), nb, ins, lens, outs))

    def debug_ntt_split(self, log_r=()):
        """zkt_debug_ntt_split: force the pass radices of the transforms above 2^10 run afterwards; () restores the policy."""
        lr = (ctypes.c_int * max(len(log_r), 3))(*log_r)
        self.check(self._L.zkt_debug_ntt_split(self._h, len(log_r), lr))

    def debug_fr_mul(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
        out = np.empty_like(a)
        self.check(self._L.zkt_debug_fr_mul(self._h, u64p(a), u64p(b), a.shape[0], u64p(out)))
        return out

    def debug_fx_op(self, which: int, op: int, records) -> np.ndarray:
        """zkt_debug_fx_op: the field routine `op` on the device, one (4 L,) u32 record per thread."""
        L_ = fx_layout(self.curve, which)[0]
        rec = _records(records, 4 * L_)
        out = np.zeros_like(rec)
        self.check(self._L.zkt_debug_fx_op(self._h, which, op, _u32p(rec), rec.shape[0], _u32p(out)))
        return out

    def debug_xyzz_op(self, op: int, records) -> np.ndarray:
        """zkt_debug_xyzz_op: the curve routine `op` on the device, one (2 (4 L + 1),) u32 record per thread."""
        w = 4 * fx_layout(self.curve, 1)[0] + 1
        rec = _records(records, 2 * w)
        out = np.zeros((rec.shape[0], w), dtype=np.uint32)
        self.check(self._L.zkt_debug_xyzz_op(self._h, op, _u32p(rec), rec.shape[0], _u32p(out)))
        return out

    def debug_grand_products(self, n: int, challenges, vectors):
        """z1, z2 evaluation vectors (zkt_debug_grand_products): challenges (4, 4) beta gamma delta epsilon; vectors: seven
        (n, 4) host arrays a b c f t h1 h2."""
        ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(4, 4)
        keep = [np.ascontiguousarray(w, dtype=np.uint64).reshape(n, 4) for w in vectors]
        assert len(keep) == 7
        ptrs = (ctypes.c_void_p * 7)(*[w.ctypes.data for w in keep])
        z1, z2 = np.empty((n, 4), dtype=np.uint64), np.empty((n, 4), dtype=np.uint64)
        self._L.zkt_debug_grand_products.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_void_p),
                                                     ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        self.check(self._L.zkt_debug_grand_products(self._h, u64p(ch), ptrs, u64p(z1), u64p(z2)))
        return z1, z2

    def debug_combine_split(self, table, f, fresh: bool = True):
        """h1, h2 (n, 4) each through the prover's round-2 code (zkt_debug_combine_split): table (table_len, 4) distinct
        values in insertion order, f (n, 4) for the loaded circuit's n; fresh=False reuses the keys the previous call or
        proof left on the device.  Montgomery words throughout."""
        t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 4)
        ff = np.ascontiguousarray(f, dtype=np.uint64).reshape(-1, 4)
        if self.circuit_log_n is None or ff.shape[0] != 1 << self.circuit_log_n:
            raise ValueError("f must hold the n elements of a circuit loaded through this Context")
        n = ff.shape[0]
        h1, h2 = np.empty((n, 4), dtype=np.uint64), np.empty((n, 4), dtype=np.uint64)
        P64 = ctypes.POINTER(ctypes.c_uint64)
        self._L.zkt_debug_combine_split.argtypes = [ctypes.c_void_p, P64, ctypes.c_size_t, P64, ctypes.c_int, P64, P64]
        self.check(self._L.zkt_debug_combine_split(self._h, u64p(t) if t.shape[0] else None, t.shape[0], u64p(ff),
                                                   1 if fresh else 0, u64p(h1), u64p(h2)))
        return h1, h2

    def debug_commit_wires_dev(self, d_variables: int, n_vars: int, d_w_l: int, d_w_r: int, d_w_o: int, n_rows: int, blinders,
                               route: int = 1, pi_pos=None):
        """zkt_debug_commit_wires_dev: the prover's round-1 commitments of the three wires for a variable map and index
        vectors in HBM (device addresses).  blinders (6, 4).  -> (xy (3, 2*fq_limbs) Montgomery limbs, is_infinity (3,),
        route taken (3,): 1 = over the wire's base table, 2 = over its table of free variables).  route 2, or any route with
        pi_pos (the proof's public-input positions), goes through zkt_debug_commit_wires_pi_dev."""
        bl = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(6, 4)
        out = np.zeros((3, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * 3)()
        took = (ctypes.c_int * 3)()
        if route == 2 or pi_pos is not None:
            pos = [int(x) for x in (pi_pos or ())]
            pi = (ctypes.c_size_t * max(len(pos), 1))(*pos)
            self._L.zkt_debug_commit_wires_pi_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                                              ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int),
                                                              ctypes.POINTER(ctypes.c_int)]
            self.check(self._L.zkt_debug_commit_wires_pi_dev(self._h, ctypes.c_void_p(d_variables), n_vars, ctypes.c_void_p(d_w_l),
                                                             ctypes.c_void_p(d_w_r), ctypes.c_void_p(d_w_o), n_rows, u64p(bl),
                                                             int(route), pi, len(pos), u64p(out), inf, took))
            return out, [bool(x) for x in inf], [int(x) for x in took]
        self._L.zkt_debug_commit_wires_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                       ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int),
                                                       ctypes.POINTER(ctypes.c_int)]
        self.check(self._L.zkt_debug_commit_wires_dev(self._h, ctypes.c_void_p(d_variables), n_vars, ctypes.c_void_p(d_w_l),
                                                      ctypes.c_void_p(d_w_r), ctypes.c_void_p(d_w_o), n_rows, u64p(bl), int(route),
                                                      u64p(out), inf, took))
        return out, [bool(x) for x in inf], [int(x) for x in took]

    def check_epk_file(self, path: str):
        """zkt_circuit_check_epk_file: None when every vector of the reference CLI's --epk file equals the loaded circuit's
        extended key as the device derives it, else (vector 0..16, first differing element or -1 for a wrong length)."""
        self._L.zkt_circuit_check_epk_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                                       ctypes.POINTER(ctypes.c_size_t)]
        vec, at = ctypes.c_int(0), ctypes.c_size_t(0)
        self.check(self._L.zkt_circuit_check_epk_file(self._h, path.encode(), ctypes.byref(vec), ctypes.byref(at)))
        if vec.value < 0:
            return None
        return vec.value, (-1 if at.value == ctypes.c_size_t(-1).value else at.value)

    # -- the keys that setup makes, and the files of the reference CLI's `Compile` -----------------------
    def circuit_export(self, lengths_only: bool = False):
        """zkt_circuit_export: the ten ProverKey polynomials of the loaded circuit as (len_k, 4) Montgomery arrays in
        zkt_circuit_load order, trimmed as DensePolynomial::from_coefficients_vec leaves them; lengths_only: the ten
        lengths, nothing downloaded."""
        P64 = ctypes.POINTER(ctypes.c_uint64)
        self._L.zkt_circuit_export.argtypes = [ctypes.c_void_p, ctypes.POINTER(P64), ctypes.POINTER(ctypes.c_size_t)]
        lens = (ctypes.c_size_t * 10)()
        if lengths_only:
            self.check(self._L.zkt_circuit_export(self._h, None, lens))
            return list(lens)
        if self.circuit_log_n is None:
            raise ValueError("circuit_export: load the circuit through this Context (entry buffers hold n elements)")
        arrs = [np.zeros((1 << self.circuit_log_n, 4), dtype=np.uint64) for _ in range(10)]
        ptrs = (P64 * 10)(*[u64p(a) for a in arrs])
        self.check(self._L.zkt_circuit_export(self._h, ptrs, lens))
        return [a[:lens[k]].copy() for k, a in enumerate(arrs)]

    def circuit_commitments(self):
        """zkt_circuit_commitments -> (commitments (10, 2*fq_limbs) Montgomery limbs, is_infinity (10,) bool): the
        VerifierKey commitments of the loaded circuit under the loaded SRS, as circuit_setup returns them."""
        self._L.zkt_circuit_commitments.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        out = np.zeros((10, 2 * self.fq_limbs), dtype=np.uint64)
        inf = (ctypes.c_int * 10)()
        self.check(self._L.zkt_circuit_commitments(self._h, u64p(out), inf))
        return out, np.array([bool(x) for x in inf])

    def circuit_export_epk(self, which: int = -1, cap: int = None):
        """zkt_circuit_export_epk -> (the seventeen lengths, vector `which` as (len, 4) Montgomery limbs or None for -1);
        cap: the element count announced for the buffer (default: the vector's length)."""
        P64 = ctypes.POINTER(ctypes.c_uint64)
        self._L.zkt_circuit_export_epk.argtypes = [ctypes.c_void_p, ctypes.c_int, P64, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        lens = (ctypes.c_size_t * 17)()
        self.check(self._L.zkt_circuit_export_epk(self._h, -1, None, 0, lens))
        if which < 0:
            return list(lens), None
        out = np.zeros((max(lens[which], 1), 4), dtype=np.uint64)
        self.check(self._L.zkt_circuit_export_epk(self._h, which, u64p(out), lens[which] if cap is None else cap, lens))
        return list(lens), out[:lens[which]]

    def check_vk_file(self, path: str):
        """zkt_circuit_check_vk_file: None when the --vk file's n and ten commitments are the loaded circuit's under the
        loaded SRS, else the first differing commitment (0 .. 9) or 10 for n."""
        self._L.zkt_circuit_check_vk_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        at = ctypes.c_int(0)
        self.check(self._L.zkt_circuit_check_vk_file(self._h, path.encode(), ctypes.byref(at)))
        return None if at.value < 0 else at.value

    def srs_save_file(self, ck_path: str, count: int = 0):
        """zkt_srs_save_file: the first `count` loaded powers (0: all) as the reference CLI's --ck file."""
        self._L.zkt_srs_save_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        self.check(self._L.zkt_srs_save_file(self._h, ck_path.encode(), count))

    def write_epk_file(self, epk_path: str):
        """zkt_circuit_write_epk_file: the loaded circuit's ExtendedProverKey streamed into the --epk file."""
        self._L.zkt_circuit_write_epk_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        self.check(self._L.zkt_circuit_write_epk_file(self._h, epk_path.encode()))

    def circuit_save_files(self, pk_path: str = None, vk_path: str = None, epk_path: str = None, pi_pos=()):
        """zkt_circuit_save_files: the --pk / --vk / --epk files of the loaded circuit (None: skipped); pi_pos: the
        public-input positions behind the vk's pi_roots, ascending."""
        pos = [int(x) for x in pi_pos]
        arr = (ctypes.c_size_t * max(len(pos), 1))(*pos)
        enc = lambda p: None if p is None else p.encode()
        self._L.zkt_circuit_save_files.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                   ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t]
        self.check(self._L.zkt_circuit_save_files(self._h, enc(pk_path), enc(vk_path), enc(epk_path), arr, len(pos)))

    def debug_eval_lincomb(self, polys, points, scalars, out_len: int):
        """zkt_debug_eval_lincomb: polys: list of (len_j, 4) arrays, points / scalars (k, 4); returns (evals (k, 4), lincomb
        (out_len, 4)).  Montgomery words throughout."""
        keep = [np.ascontiguousarray(p_, dtype=np.uint64).reshape(-1, 4) for p_ in polys]
        k = len(keep)
        P64 = ctypes.POINTER(ctypes.c_uint64)
        ptrs = (P64 * k)(*[u64p(a) for a in keep])
        lens = (ctypes.c_size_t * k)(*[a.shape[0] for a in keep])
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(k, 4)
        scs = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(k, 4)
        ev = np.empty((k, 4), dtype=np.uint64)
        lc = np.empty((out_len, 4), dtype=np.uint64)
        self._L.zkt_debug_eval_lincomb.argtypes = [ctypes.c_void_p, ctypes.POINTER(P64), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
                                                   P64, P64, P64, P64, ctypes.c_size_t]
        self.check(self._L.zkt_debug_eval_lincomb(self._h, ptrs, lens, k, u64p(pts), u64p(scs), u64p(ev), u64p(lc), out_len))
        return ev, lc

    def debug_open_witness(self, coeffs, z) -> np.ndarray:
        """(p(X) - p(z)) / (X - z) (zkt_debug_open_witness): coeffs (len, 4), z (4,), Montgomery words."""
        p_ = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(4)
        out = np.empty((p_.shape[0] - 1, 4), dtype=np.uint64)
        self._L.zkt_debug_open_witness.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        self.check(self._L.zkt_debug_open_witness(self._h, u64p(p_), p_.shape[0], u64p(zz), u64p(out)))
        return out

    def set_quotient_route(self, mode: int = 0):
        """zkt_ctx_set_quotient_route: 0 automatic (three classes for single-GPU circuits of 2^18 rows and more), 1 the
        quotient on three classes of the 4n coset, 2 on the whole coset"""
        self._L.zkt_ctx_set_quotient_route.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.check(self._L.zkt_ctx_set_quotient_route(self._h, int(mode)))

    def set_fused_passes(self, mode: int = 0):
        """zkt_ctx_set_fused_passes: 0 automatic (fused), 1 the fused streaming passes of rounds 3 and 5 and of the blinding,
        2 one launch per step (the sequence the fused one is tested against)"""
        self._L.zkt_ctx_set_fused_passes.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.check(self._L.zkt_ctx_set_fused_passes(self._h, int(mode)))

    def debug_quotient_top(self):
        """zkt_debug_quotient_top -> (u (6, 4) Montgomery words, whether the last proof took the quotient on classes)"""
        u = np.zeros((6, 4), dtype=np.uint64)
        on = ctypes.c_int(0)
        self._L.zkt_debug_quotient_top.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        self.check(self._L.zkt_debug_quotient_top(self._h, u64p(u), ctypes.byref(on)))
        return u, bool(on.value)

    def debug_quotient_coeffs(self, count: int) -> np.ndarray:
        """zkt_debug_quotient_coeffs: the first `count` coefficients of the quotient as the last proof left them"""
        out = np.zeros((count, 4), dtype=np.uint64)
        self._L.zkt_debug_quotient_coeffs.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]
        self.check(self._L.zkt_debug_quotient_coeffs(self._h, u64p(out), int(count)))
        return out

    def debug_quotient(self, n: int, challenges, wit, pi_pos=(), pi_vals=None) -> np.ndarray:
        """The quotient kernel alone over the loaded circuit (zkt_debug_quotient): challenges (5, 4) alpha beta gamma
        delta epsilon; wit: nine (4n, 4) host arrays a b c pi z1 z2 t h1 h2 (wit[3] may be None with public inputs
        given as positions + values).  Montgomery words throughout."""
        ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(5, 4)
        keep = [None if w is None else np.ascontiguousarray(w, dtype=np.uint64).reshape(4 * n, 4) for w in wit]
        assert len(keep) == 9
        ptrs = (ctypes.c_void_p * 9)(*[None if w is None else w.ctypes.data for w in keep])
        pos = np.ascontiguousarray(list(pi_pos), dtype=np.uint64)
        vals = np.ascontiguousarray(pi_vals if len(pos) else np.zeros((0, 4)), dtype=np.uint64).reshape(-1, 4)
        out = np.empty((4 * n, 4), dtype=np.uint64)
        self.check(self._L.zkt_debug_quotient(self._h, u64p(ch), ptrs, u64p(pos) if len(pos) else None,
                                              u64p(vals) if len(pos) else None, len(pos), u64p(out)))
        return out
