"""ctypes binding of libdecomp_hip.so (the C ABI declared in include/decomp_hip.h).

The HIP library IS the compute path: there is no CPU fallback.  If the shared object
is missing or no MI355X is visible, the first call raises (loudly) instead of
computing somewhere else.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libdecomp_hip.so')

OK = 0
ERR_NAMES = {-1: 'DCP_ERR_INVALID', -2: 'DCP_ERR_HIP', -3: 'DCP_ERR_NOMEM',
             -4: 'DCP_ERR_INTERNAL', -5: 'DCP_ERR_UNSUPPORTED', -6: 'DCP_ERR_REF_TYPEERROR',
             -7: 'DCP_ERR_COMM'}
LIK_L2, LIK_KL, LIK_BETA = 0, 1, 2
PROF_NLABELS = 10
PROF_XUPDATE, PROF_STATS = 2, 4
LASSO_ISTA, LASSO_ACC_ISTA, LASSO_FISTA, LASSO_CD = 0, 1, 2, 3
LASSO_PARALLEL_CD, LASSO_ADMM = 4, 5
LASSO_OMP = 6            # dcp_dict_* only: orthogonal matching pursuit as the inner coder
LASSO_POSITIVE = 0x100
ERR_REF_TYPEERROR = -6
ERR_COMM = -7
COMM_ID_BYTES = 128
# int fn(void* buf, int64 count, int dtype, void* hip_stream, void* user)  (dcp_comm_set_external)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)

_c_int, _c_i64, _c_vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_c_f32, _c_f64 = ctypes.c_float, ctypes.c_double
_P = ctypes.POINTER

# The C ABI by family: (stem, suffixes, argtypes[, restype]).  A family is one prototype of include/decomp_hip.h in the
# dtypes it exists in (None: a single function without a suffix); restype defaults to int.  The handle and every
# device array travel as void*.  Where the C type follows the dtype the list names it: _REAL is the float / double
# scalar of the dtype, _P_REAL a host pointer to it.  tests/test_abi.py parses the header and checks every return
# type, argument count and argument type of the resulting SIGNATURES against it.
_ALL = ('f32', 'f64', 'c64', 'c128')
_REALS = ('f32', 'f64')
_REAL, _P_REAL = object(), object()
_REAL_OF = {'f32': _c_f32, 'f64': _c_f64, 'c64': _c_f32, 'c128': _c_f64}
_P_INT, _P_F64 = _P(_c_int), _P(_c_f64)
_NFK = [_c_i64] * 3                 # N, F, K
_TM = [_c_i64] * 5 + [_c_int]       # B, T, S, N, stride, padding
_TM_MC = [_c_i64] * 6 + [_c_int]    # B, T, Ch, S, N, stride, padding
_MASKED = [_c_vp] * 3 + [_c_int, _c_vp, _c_vp] + _NFK   # h, Y, mask, mask_ndim, two more arrays, N, F, K

_FAMILIES = [
    # lifetime, communicator, profile
    ('dcp_create', None, [_P(_c_vp), _c_int]),
    ('dcp_destroy', None, [_c_vp]),
    ('dcp_set_stream', None, [_c_vp, _c_vp]),
    ('dcp_last_error_string', None, [_c_vp], ctypes.c_char_p),
    ('dcp_build_info', None, [], ctypes.c_char_p),
    ('dcp_comm_unique_id', None, [_c_vp, _c_i64]),
    ('dcp_comm_init', None, [_c_vp, _c_vp, _c_int, _c_int]),
    ('dcp_comm_destroy', None, [_c_vp]),
    ('dcp_comm_set_external', None, [_c_vp] * 3 + [_c_int, _c_int]),
    ('dcp_memcpy', None, [_c_vp] * 3 + [_c_i64]),
    ('dcp_comm_info', None, [_c_vp, _P_INT, _P_INT]),
    ('dcp_comm_allreduce_sum', _REALS, [_c_vp, _c_vp, _c_i64]),
    ('dcp_profile_enable', None, [_c_vp, _c_int]),
    ('dcp_profile_reset', None, [_c_vp]),
    ('dcp_profile_select', None, [_c_vp, ctypes.c_uint]),
    ('dcp_profile_read', None, [_c_vp, _c_int, _P_F64, _P(_c_i64)]),
    ('dcp_profile_label_name', None, [_c_int], ctypes.c_char_p),
    # utilities and test hooks
    ('dcp_l2_normalize', _ALL, [_c_vp, _c_vp, _c_i64, _c_i64, _c_int]),
    ('dcp_l2_normalize_diff', _REALS, [_c_vp] * 4 + [_c_i64, _c_i64, _c_int, _P_F64]),
    ('dcp_count_negative', _REALS, [_c_vp, _c_vp, _c_i64, _P(_c_i64)]),
    ('dcp_gershgorin', _ALL, [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp]),
    ('dcp_inv', _ALL, [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp]),
    ('dcp_mu_quotient', _REALS, [_c_vp] * 4 + [_c_i64, _c_i64, _c_vp]),
    ('dcp_axpby', _REALS, [_c_vp, _c_i64, _c_f64, _c_vp, _c_f64, _c_vp]),
    ('dcp_gemm', _ALL, [_c_vp, _c_int] + [_c_vp] * 3 + _NFK + [_c_int, _c_int]),
    ('dcp_gemm_bf16x6', ('f32',), [_c_vp, _c_int] + [_c_vp] * 3 + _NFK + [_c_int]),
    ('dcp_gemm_bf16x6_seg', ('f32',), [_c_vp, _c_int] + [_c_vp] * 4 + [_c_i64] * 4 + [_c_int]),
    ('dcp_gemm_bf16x6_tier', None, [_c_int] + [_c_i64] * 4 + [_c_int]),
    ('dcp_set_f32_product_mode', None, [_c_vp, _c_int]),
    ('dcp_debug_tn_plain', None, [_c_int]),
    ('dcp_debug_gemm_route', None, [_c_int, _c_int] + [_c_i64] * 4 + [_c_int] * 5 + [_c_vp]),
    ('dcp_calib_read', ('f32',), [_c_vp, _c_vp, _c_i64, _c_i64, _c_int, _c_vp]),
    # row movers
    ('dcp_gather_rows_bytes', None, [_c_vp] * 3 + [_c_i64, _c_i64, _c_vp]),
    ('dcp_scatter_rows_bytes', None, [_c_vp] * 3 + [_c_i64, _c_i64, _c_vp]),
    ('dcp_dict_prefetch_rows_bytes', None, [_c_vp] * 3 + [_c_i64, _c_i64, _c_vp]),
    ('dcp_gather_rows', _ALL, [_c_vp] * 3 + [_c_i64, _c_i64, _c_vp]),
    # NMF: tol and the host scalars it is compared with are float in f32, double in f64
    ('dcp_nmf_mu', _REALS, [_c_vp] * 5 + _NFK + [_c_int, _REAL, _c_int, _P_INT, _P_REAL, _P_REAL]),
    ('dcp_nmf_mu_sharded', _REALS, [_c_vp] * 5 + _NFK + [_c_int, _REAL, _c_int, _P_INT, _P_REAL]),
    ('dcp_nmf_hals', _REALS, [_c_vp] * 4 + _NFK + [_REAL, _c_int, _P_INT, _P_REAL, _P_REAL]),
    ('dcp_nmf_hals_sharded', _REALS, [_c_vp] * 4 + _NFK + [_REAL, _c_int, _P_INT, _P_REAL]),
    ('dcp_nmf_emhals', _REALS, [_c_vp] * 5 + _NFK + [_REAL, _c_int, _P_INT, _P_REAL, _P_REAL]),
    ('dcp_nmf_emhals_sharded', _REALS, [_c_vp] * 5 + _NFK + [_REAL, _c_int, _P_INT, _P_REAL]),
    ('dcp_nmf_impute', _REALS, [_c_vp] * 5 + _NFK + [_c_vp]),
    ('dcp_nmf_hals_stats', _REALS, [_c_vp] * 5 + _NFK + [_c_vp]),
    ('dcp_nmf_hals_update', _REALS, [_c_vp] * 5 + _NFK + [_c_vp, _c_vp]),
    ('dcp_nn_cd_sweep', _REALS, [_c_vp] * 5 + [_c_i64, _c_i64, _c_int]),
    ('dcp_nmf_mu_stats_width', None, [_c_i64, _c_i64, _c_int, _c_int], _c_i64),
    ('dcp_nmf_mu_stats', _REALS, [_c_vp] * 6 + _NFK + [_c_int, _c_vp]),
    ('dcp_nmf_mask_bits_words', None, [_c_i64, _c_i64], _c_i64),
    ('dcp_nmf_mask_prepare', _REALS, [_c_vp] * 3 + [_c_i64, _c_i64, _c_vp, _c_vp, _P_INT]),
    ('dcp_nmf_mu_stats_prepared', _REALS, [_c_vp] * 7 + _NFK + [_c_int, _c_vp]),
    ('dcp_nmf_mu_update', _REALS, [_c_vp] * 4 + [_c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp]),
    ('dcp_nmf_grads', _REALS, [_c_vp] * 5 + _NFK + [_c_int, _c_int, _c_vp, _c_vp]),
    ('dcp_nmf_grad_x', _REALS, [_c_vp] * 5 + _NFK + [_c_int, _c_vp, _c_vp]),
    ('dcp_nmf_gauss_logp', _REALS, [_c_vp] * 5 + _NFK + [_c_f64, _P_F64]),
    ('dcp_set_nmf_beta', None, [_c_vp, _c_f64]),
    ('dcp_set_nmf_penalty', None, [_c_vp, _c_f64, _c_f64]),
    ('dcp_nmf_beta_divergence', _REALS, [_c_vp] * 5 + _NFK + [_P_F64]),
    ('dcp_nmf_apply', _REALS, [_c_vp] * 4 + [_c_f64, _c_vp, _c_i64, _c_i64, _P_F64]),
    ('dcp_nmf_residual', _REALS, [_c_vp] * 5 + _NFK + [_P_F64]),
    # LASSO, OMP, K-SVD
    ('dcp_lasso', _ALL, _MASKED + [_c_f64, _c_f64, _c_int, _c_int, _c_int, _P_INT]),
    ('dcp_lasso_pcd', _ALL, _MASKED + [_c_f64, _c_f64, _c_int, _c_int, _c_vp, _c_i64, _P_INT]),
    ('dcp_lasso_admm', _ALL, _MASKED + [_c_f64, _c_f64, _c_int, _c_int, _c_f64, _P_INT]),
    ('dcp_omp', _ALL, [_c_vp] * 4 + _NFK + [_c_int, _c_f64, _P_INT]),
    ('dcp_omp_gram', _ALL, [_c_vp] * 5 + [_c_i64, _c_i64, _c_int, _c_f64, _P_INT]),
    ('dcp_omp_mask', _ALL, _MASKED + [_c_int, _c_f64, _c_int, _P_INT]),
    ('dcp_ksvd_sweep', _ALL, [_c_vp] * 4 + _NFK + [_c_int, _P_F64]),
    ('dcp_ksvd_step', _ALL, [_c_vp] * 4 + _NFK + [_c_int, _c_f64, _P_F64, _P_INT]),
    ('dcp_ksvd_mask_sweep', _ALL, _MASKED + [_c_int, _P_F64]),
    ('dcp_ksvd_mask_step', _ALL, _MASKED + [_c_int, _c_f64, _c_int, _P_F64, _P_INT]),
    ('dcp_ksvd_clean', _ALL, _MASKED + [_c_f64, _P_INT, _P_INT]),
    ('dcp_ksvd_clean_step', _ALL, _MASKED + [_c_int, _c_f64, _c_int, _P_F64, _P_INT, _c_f64, _c_f64, _P_INT]),
    # dictionary learning
    ('dcp_dict_set_pcd_order', None, [_c_vp, _c_vp, _c_i64, _c_i64]),
    ('dcp_dict_stats', _ALL, [_c_vp] * 4 + _NFK + [_c_f64, _c_int, _c_int, _c_f64, _c_vp, _P_INT]),
    ('dcp_dict_update', _ALL, [_c_vp, _c_vp, _c_f64] + [_c_vp] * 4 + [_c_i64, _c_i64, _c_vp]),
    ('dcp_dict_step', _ALL, [_c_vp] * 7 + _NFK + [_c_f64, _c_f64, _c_int, _c_int, _c_f64, _P_F64, _P_INT]),
    ('dcp_dict_step_async', _ALL, [_c_vp] * 7 + _NFK + [_c_f64, _c_f64, _c_int, _c_int, _c_f64, _c_vp, _P_INT]),
    ('dcp_dict_mask_step', _ALL, [_c_vp] * 8 + _NFK + [_c_f64, _c_f64, _c_int, _c_int, _c_f64, _P_F64, _P_INT]),
    # template matching; the dcp_tm_mc_* twins carry Ch after T
    ('dcp_tm_temp2mat', _ALL, [_c_vp, _c_vp] + _TM[1:] + [_c_vp]),
    ('dcp_tm_coef2mat', _ALL, [_c_vp, _c_vp] + _TM + [_c_vp]),
    ('dcp_tm_predict', _ALL, [_c_vp] * 3 + _TM + [_c_vp]),
    ('dcp_tm_mc_predict', _ALL, [_c_vp] * 3 + _TM_MC + [_c_vp]),
    ('dcp_tm_lasso', _ALL, [_c_vp] * 4 + _TM + [_c_f64, _c_f64, _c_int, _c_int, _c_int, _P_INT]),
    ('dcp_tm_mc_lasso', _ALL, [_c_vp] * 4 + _TM_MC + [_c_f64, _c_f64, _c_int, _c_int, _c_int, _P_INT]),
    ('dcp_tm_pursuit', _ALL, [_c_vp] * 4 + _TM + [_c_i64, _c_f64, _c_int, _P_INT]),
    ('dcp_tm_mc_pursuit', _ALL, [_c_vp] * 4 + _TM_MC + [_c_i64, _c_f64, _c_int, _P_INT]),
    ('dcp_tm_omp', _ALL, [_c_vp] * 4 + _TM + [_c_i64, _c_f64, _P_INT]),
    ('dcp_tm_mc_omp', _ALL, [_c_vp] * 4 + _TM_MC + [_c_i64, _c_f64, _P_INT]),
    ('dcp_tm_pursuit_lds_atoms', _ALL, []),
    ('dcp_tm_omp_lds_atoms', _ALL, []),
    ('dcp_tm_mc_template_block', _ALL, []),
    ('dcp_tm_mc_channels_per_pass', _ALL, [_c_i64, _c_i64]),
    ('dcp_tm_dstep', _ALL, [_c_vp] * 6 + _TM + [_c_int, _P_F64]),
    ('dcp_tm_dstep_events', _ALL, [_c_vp] * 6 + _TM + [_c_int, _c_i64, _P_F64]),
    ('dcp_tm_mc_dstep_events', _ALL, [_c_vp] * 6 + _TM_MC + [_c_int, _c_i64, _P_F64]),
    # ... m, B, T, [Ch,] S, N, w, stride, padding ...
    ('dcp_tm_gather_windows', _ALL, [_c_vp] * 5 + [_c_i64] * 7 + [_c_int, _c_vp, _c_vp]),
    ('dcp_tm_mc_gather_windows', _ALL, [_c_vp] * 5 + [_c_i64] * 8 + [_c_int, _c_vp, _c_vp]),
    ('dcp_tm_scatter_windows', _ALL, [_c_vp] * 5 + [_c_i64] * 7 + [_c_int]),
]


def _signatures():
    """name -> (restype, argtypes) for every entry point of every family."""
    out = {}
    for stem, suffixes, args, *res in _FAMILIES:
        for sfx in suffixes or (None,):
            real = _REAL_OF.get(sfx)
            of = {_REAL: real, _P_REAL: real and _P(real)}
            name = stem if sfx is None else '%s_%s' % (stem, sfx)
            assert name not in out, name
            out[name] = (res[0] if res else _c_int, [of.get(a, a) for a in args])
    return out


SIGNATURES = _signatures()

_lib = None
_lock = threading.Lock()
_handles = {}


class HipLibraryError(RuntimeError):
    """The HIP library is missing, failed to load, or a call into it failed."""


def load():
    """Load libdecomp_hip.so (once) and declare every entry point's signature."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                'libdecomp_hip.so not found at %s. Build it with `make` (or '
                '`python -c "import __graft_entry__ as g; g.build()"`). decomp_amd has no '
                'CPU fallback: the HIP library is the compute path.' % LIB_PATH)
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise HipLibraryError('cannot load %s: %s' % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return _lib


def handle(device):
    """The per-device library handle (created on first use)."""
    lib = load()
    with _lock:
        h = _handles.get(device)
        if h is None:
            out = _c_vp()
            rc = lib.dcp_create(ctypes.byref(out), int(device))
            if rc != OK or not out.value:
                raise HipLibraryError(
                    'dcp_create(device=%d) failed (%s): no usable HIP device. decomp_amd '
                    'computes only on the GPU.' % (device, ERR_NAMES.get(rc, rc)))
            h = out
            _handles[device] = h
        return h


def check(h, rc, what):
    if rc != OK:
        msg = load().dcp_last_error_string(h)
        raise HipLibraryError('%s failed: %s (%s)' % (
            what, ERR_NAMES.get(rc, rc), msg.decode() if msg else ''))
