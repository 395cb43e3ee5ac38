"""ctypes mirror of include/hhmm.h (ABI version 2).

Field order and types must match the C structs exactly; tests/test_abi.py
checks the sizes against offsets parsed from the header.
"""
import ctypes as C

ABI_VERSION = 2

# hhmm_status
OK = 0
WARN_PAIR_FAILURES = 1
ERR_INVALID_ARGUMENT = -1
ERR_OUT_OF_MEMORY = -2
ERR_HIP = -3
ERR_UNSUPPORTED = -4
ERR_NO_DEVICE = -5

PAIR_OK = 0
PAIR_INVALID_BACKPOINTER = 1
PAIR_INVALID_DATA = 2  # hhmm_run_device: the series breaks a data-block bound (include/hhmm.h)

MODELS = {
    "hmm": 1,                    # hmm/stan/hmm.stan
    "hmm-multinom": 2,           # hmm/stan/hmm-multinom.stan
    "hmm-multinom-semisup": 3,   # hmm/stan/hmm-multinom-semisup.stan
    "iohmm-reg": 4,              # iohmm-reg/stan/iohmm-reg.stan
    "iohmm-mix": 5,              # iohmm-mix/stan/iohmm-mix.stan
    "iohmm-hmix": 6,             # iohmm-mix/stan/iohmm-hmix.stan
    "iohmm-hmix-lite": 7,        # iohmm-mix/stan/iohmm-hmix-lite.stan
    "hhmm-tayal2009": 8,         # tayal2009/stan/hhmm-tayal2009.stan
    "hhmm-tayal2009-lite": 9,    # tayal2009/stan/hhmm-tayal2009-lite.stan
}

PAIR_GRID = 0
PAIR_ZIP = 1
PAIR_BLOCK = 2

# hhmm_request.flags
FLAG_SCAN_AUTO = 0
FLAG_SCAN_FORCE = 1 << 0
FLAG_SCAN_OFF = 1 << 1
FLAG_NO_FUSE = 1 << 2
FLAG_VIT_LANES = 1 << 3
FLAG_VIT_STATES = 1 << 4
FLAG_FUSED = 1 << 5
FLAG_VIT_SCAN = 1 << 6
FLAG_VIT_SCAN_OFF = 1 << 7
FLAG_FB_SPLIT = 1 << 16
FLAG_LKM_MFMA = 1 << 17
FLAG_VFB = 1 << 18
FLAG_VFB_OFF = 1 << 19
DEVICE_SET = -2  # hhmm_request.device: shard over the device set (HHMM_DEVICE_SET)


def flag_scan_chunk_log2(n):
    """T-chunk length 2^n for the parallel scan (HHMM_FLAG_SCAN_CHUNK_LOG2)."""
    return int(n) << 8


def flag_host_chunks(n):
    """hhmm_run's host pipeline in n chunks (HHMM_FLAG_HOST_CHUNKS; 0 = automatic)."""
    return (int(n) & 0xFF) << 20

OUT = {
    "loglik": 1 << 0,
    "unalpha_tk": 1 << 1,
    "alpha_tk": 1 << 2,
    "unbeta_tk": 1 << 3,
    "beta_tk": 1 << 4,
    "ungamma_tk": 1 << 5,
    "gamma_tk": 1 << 6,
    "zstar_t": 1 << 7,
    "logp_zstar": 1 << 8,
    "oblik_tk": 1 << 9,
    "oblik_t": 1 << 10,
    "z_ffbs": 1 << 11,
    "alpha_tk_oos": 1 << 12,
    "unalpha_tk_oos": 1 << 13,
    "logA_ij": 1 << 14,
    "hatpi_tk": 1 << 15,
    "hatz_t": 1 << 16,
    "hatl_t": 1 << 17,
    "hatx_t": 1 << 18,
}

I32P = C.POINTER(C.c_int32)
F64P = C.POINTER(C.c_double)


class Data(C.Structure):
    _fields_ = [
        ("n_series", C.c_int64),
        ("T_max", C.c_int32),
        ("K", C.c_int32),
        ("L", C.c_int32),
        ("M", C.c_int32),
        ("G", C.c_int32),
        ("T_oos_max", C.c_int32),
        ("T", C.c_void_p),
        ("x_int", C.c_void_p),
        ("x_real", C.c_void_p),
        ("g", C.c_void_p),
        ("sign", C.c_void_p),
        ("u", C.c_void_p),
        ("T_oos", C.c_void_p),
        ("x_oos", C.c_void_p),
        ("sign_oos", C.c_void_p),
        ("hyperparams", C.c_void_p),
    ]


class Draws(C.Structure):
    _fields_ = [
        ("n_draws", C.c_int64),
        ("p_1k", C.c_void_p),
        ("A_ij", C.c_void_p),
        ("phi_k", C.c_void_p),
        ("mu_k", C.c_void_p),
        ("sigma_k", C.c_void_p),
        ("w_km", C.c_void_p),
        ("b_km", C.c_void_p),
        ("s_k", C.c_void_p),
        ("lambda_kl", C.c_void_p),
        ("mu_kl", C.c_void_p),
        ("s_kl", C.c_void_p),
        ("p_11", C.c_void_p),
        ("A_row", C.c_void_p),
    ]


class Request(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("model", C.c_int32),
        ("pairing", C.c_int32),
        ("outputs", C.c_uint32),
        ("data", Data),
        ("draws", Draws),
        ("ffbs_u", C.c_void_p),
        ("device", C.c_int32),
        ("flags", C.c_int32),
        ("hat_rand", C.c_void_p),
    ]


class Result(C.Structure):
    _fields_ = [
        ("loglik", C.c_void_p),
        ("unalpha_tk", C.c_void_p),
        ("alpha_tk", C.c_void_p),
        ("unbeta_tk", C.c_void_p),
        ("beta_tk", C.c_void_p),
        ("ungamma_tk", C.c_void_p),
        ("gamma_tk", C.c_void_p),
        ("zstar_t", C.c_void_p),
        ("logp_zstar", C.c_void_p),
        ("oblik_tk", C.c_void_p),
        ("oblik_t", C.c_void_p),
        ("z_ffbs", C.c_void_p),
        ("alpha_tk_oos", C.c_void_p),
        ("unalpha_tk_oos", C.c_void_p),
        ("logA_ij", C.c_void_p),
        ("pair_status", C.c_void_p),
        ("hatpi_tk", C.c_void_p),
        ("hatz_t", C.c_void_p),
        ("hatl_t", C.c_void_p),
        ("hatx_t", C.c_void_p),
    ]


# include/hhmm_summary.h
SUMMARY_MAX_PROBS = 16
SUMMARY_MAX_DRAWS = 16384


class SummaryRequest(C.Structure):
    _fields_ = [
        ("n_series", C.c_int64),
        ("n_draws", C.c_int64),
        ("T_max", C.c_int32),
        ("K", C.c_int32),
        ("T", C.c_void_p),
        ("n_probs", C.c_int32),
        ("reserved", C.c_int32),
        ("probs", C.c_double * SUMMARY_MAX_PROBS),
        ("argmax_prob", C.c_double),
        ("values_f64", C.c_void_p),
        ("values_i32", C.c_void_p),
    ]


class SummarySpec(C.Structure):
    _fields_ = [
        ("n_probs", C.c_int32),
        ("summarise", C.c_uint32),
        ("argmax", C.c_uint32),
        ("reserved", C.c_int32),
        ("probs", C.c_double * SUMMARY_MAX_PROBS),
        ("argmax_prob", C.c_double),
    ]


class SummaryResult(C.Structure):
    _fields_ = [
        ("quantiles", C.c_void_p * 32),
        ("argmax", C.c_void_p * 32),
    ]


# include/hhmm_estep.h
class EstepResult(C.Structure):
    _fields_ = [
        ("loglik", C.c_void_p),
        ("n_1k", C.c_void_p),
        ("xi_ij", C.c_void_p),
        ("c_kl", C.c_void_p),
        ("w_k", C.c_void_p),
        ("s1_k", C.c_void_p),
        ("s2_k", C.c_void_p),
        ("pair_status", C.c_void_p),
    ]


# include/hhmm_pointwise.h
class PointwiseResult(C.Structure):
    _fields_ = [
        ("loglik", C.c_void_p),
        ("lpd_t", C.c_void_p),
        ("mean_t", C.c_void_p),
        ("var_t", C.c_void_p),
        ("lp_t", C.c_void_p),
        ("pair_status", C.c_void_p),
    ]


# include/hhmm_psis.h
PSIS_MAX_DRAWS = 16384


class PsisResult(C.Structure):
    _fields_ = [
        ("pw", PointwiseResult),
        ("elpd_t", C.c_void_p),
        ("khat_t", C.c_void_p),
        ("neff_t", C.c_void_p),
    ]


def _embedded(name):
    return property(lambda self: getattr(self.pw, name), lambda self, v: setattr(self.pw, name, v))


for _name, _ctype in PointwiseResult._fields_:  # res.lpd_t is res.pw.lpd_t: the helpers of _stats set fields by name
    setattr(PsisResult, _name, _embedded(_name))


class PsisCellsRequest(C.Structure):
    _fields_ = [
        ("n_series", C.c_int64),
        ("n_draws", C.c_int64),
        ("T_max", C.c_int32),
        ("reserved", C.c_int32),
        ("T", C.c_void_p),
        ("lr", C.c_void_p),
        ("lp", C.c_void_p),
    ]


# include/hhmm_estep_io.h
class EstepIoResult(C.Structure):
    _fields_ = [
        ("loglik", C.c_void_p),
        ("n_1k", C.c_void_p),
        ("gw_km", C.c_void_p),
        ("n_k", C.c_void_p),
        ("uu_kmm", C.c_void_p),
        ("ux_km", C.c_void_p),
        ("xx_k", C.c_void_p),
        ("n_kl", C.c_void_p),
        ("sx_kl", C.c_void_p),
        ("sxx_kl", C.c_void_p),
        ("pair_status", C.c_void_p),
    ]


# Data-block fields (name -> (ctype kind, shape code)).  Shape codes use
# N = series, T = T_max, M, To = T_oos_max.
DATA_ARRAYS = {
    "T": ("i32", "N"),
    "x_int": ("i32", "NT"),
    "x_real": ("f64", "NT"),
    "g": ("i32", "NT"),
    "sign": ("i32", "NT"),
    "u": ("f64", "NTM"),
    "T_oos": ("i32", "N"),
    "x_oos": ("i32", "NTo"),
    "sign_oos": ("i32", "NTo"),
    "hyperparams": ("f64", "9"),
}

DRAW_ARRAYS = {
    "p_1k": "SK",
    "A_ij": "SKK",
    "phi_k": "SKL",
    "mu_k": "SK",
    "sigma_k": "SK",
    "w_km": "SKM",
    "b_km": "SKM",
    "s_k": "SK",
    "lambda_kl": "SKL",
    "mu_kl": "SKL",
    "s_kl": "SKL",
    "p_11": "S",
    "A_row": "S22",
}

# result field -> (dtype, shape code) ; P = pairs
RESULT_ARRAYS = {
    "loglik": ("f64", "P"),
    "unalpha_tk": ("f64", "PTK"),
    "alpha_tk": ("f64", "PTK"),
    "unbeta_tk": ("f64", "PTK"),
    "beta_tk": ("f64", "PTK"),
    "ungamma_tk": ("f64", "PTK"),
    "gamma_tk": ("f64", "PTK"),
    "zstar_t": ("i32", "PTz"),
    "logp_zstar": ("f64", "P"),
    "oblik_tk": ("f64", "PTK"),
    "oblik_t": ("f64", "PT"),
    "z_ffbs": ("i32", "PT"),
    "alpha_tk_oos": ("f64", "PToK"),
    "unalpha_tk_oos": ("f64", "PToK"),
    "logA_ij": ("f64", "PTK"),
    "hatpi_tk": ("f64", "PTK"),
    "hatz_t": ("i32", "PT"),
    "hatl_t": ("i32", "PT"),
    "hatx_t": ("f64", "PT"),
}


def declare(lib):
    """Attach argtypes / restypes of the public entry points."""
    RP = C.POINTER(Request)
    SP = C.POINTER(Result)
    lib.hhmm_version.restype = C.c_char_p
    lib.hhmm_last_error.restype = C.c_char_p
    lib.hhmm_num_pairs.argtypes = [RP]
    lib.hhmm_num_pairs.restype = C.c_int64
    lib.hhmm_validate.argtypes = [RP, SP, C.c_int]
    lib.hhmm_validate.restype = C.c_int
    lib.hhmm_init.argtypes = [C.c_int]
    lib.hhmm_init.restype = C.c_int
    lib.hhmm_shutdown.restype = C.c_int
    if hasattr(lib, "hhmm_init_devices"):  # absent from libraries built before the device set (A/B variants)
        lib.hhmm_init_devices.argtypes = [C.POINTER(C.c_int32), C.c_int]
        lib.hhmm_init_devices.restype = C.c_int
        lib.hhmm_device_set.argtypes = [C.POINTER(C.c_int32), C.c_int]
        lib.hhmm_device_set.restype = C.c_int
    lib.hhmm_run.argtypes = [RP, SP]
    lib.hhmm_run.restype = C.c_int
    lib.hhmm_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_workspace_size.restype = C.c_int
    lib.hhmm_run_device.argtypes = [RP, SP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_run_device.restype = C.c_int
    lib.hhmm_selftest_cr_log.argtypes = [F64P, F64P, C.c_int64]
    lib.hhmm_selftest_cr_log.restype = C.c_int
    lib.hhmm_selftest_cr_exp.argtypes = [F64P, F64P, C.c_int64]
    lib.hhmm_selftest_cr_exp.restype = C.c_int
    lib.hhmm_selftest_det_log.argtypes = [F64P, F64P, C.c_int64]
    lib.hhmm_selftest_det_log.restype = C.c_int
    lib.hhmm_selftest_det_exp.argtypes = [F64P, F64P, C.c_int64]
    lib.hhmm_selftest_det_exp.restype = C.c_int
    lib.hhmm_selftest_shards.argtypes = [RP, SP, C.c_int]
    lib.hhmm_selftest_shards.restype = C.c_int
    lib.hhmm_selftest_pipeline.argtypes = [RP, SP, C.c_int, C.c_int]
    lib.hhmm_selftest_pipeline.restype = C.c_int
    if hasattr(lib, "hhmm_selftest_plan"):  # absent from libraries built before the launch plan (A/B variants)
        lib.hhmm_selftest_plan.argtypes = [RP, C.c_char_p, C.c_size_t]
        lib.hhmm_selftest_plan.restype = C.c_int
    QP = C.POINTER(SummaryRequest)
    lib.hhmm_summary.argtypes = [QP, C.c_void_p, C.c_void_p, C.c_int]
    lib.hhmm_summary.restype = C.c_int
    lib.hhmm_summary_device.argtypes = [QP, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hhmm_summary_device.restype = C.c_int
    lib.hhmm_run_summary.argtypes = [RP, C.POINTER(SummarySpec), SP, C.POINTER(SummaryResult)]
    lib.hhmm_run_summary.restype = C.c_int
    EP = C.POINTER(EstepResult)
    lib.hhmm_estep_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_estep_workspace_size.restype = C.c_int
    lib.hhmm_estep_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_estep_device.restype = C.c_int
    lib.hhmm_estep.argtypes = [RP, EP]
    lib.hhmm_estep.restype = C.c_int
    lib.hhmm_estep_large_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_estep_large_workspace_size.restype = C.c_int
    lib.hhmm_estep_large_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_estep_large_device.restype = C.c_int
    lib.hhmm_estep_large.argtypes = [RP, EP]
    lib.hhmm_estep_large.restype = C.c_int
    # the same header: the E-step as a parallel scan over T, and the schedule "auto" follows
    lib.hhmm_estep_scan_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_estep_scan_workspace_size.restype = C.c_int
    lib.hhmm_estep_scan_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_estep_scan_device.restype = C.c_int
    lib.hhmm_estep_scan.argtypes = [RP, EP]
    lib.hhmm_estep_scan.restype = C.c_int
    lib.hhmm_estep_scan_plan.argtypes = [RP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.hhmm_estep_scan_plan.restype = C.c_int
    # include/hhmm_gibbs.h (the result struct is the E-step's)
    lib.hhmm_draw_stats_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_draw_stats_workspace_size.restype = C.c_int
    lib.hhmm_draw_stats_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_draw_stats_device.restype = C.c_int
    lib.hhmm_draw_stats.argtypes = [RP, EP]
    lib.hhmm_draw_stats.restype = C.c_int
    # the same header: hmm-multinom and hmm at 8 < K <= 32
    lib.hhmm_draw_stats_large_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_draw_stats_large_workspace_size.restype = C.c_int
    lib.hhmm_draw_stats_large_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_draw_stats_large_device.restype = C.c_int
    lib.hhmm_draw_stats_large.argtypes = [RP, EP]
    lib.hhmm_draw_stats_large.restype = C.c_int
    # include/hhmm_gibbs_gauss.h (the result struct is the E-step's)
    lib.hhmm_draw_stats_gauss_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_draw_stats_gauss_workspace_size.restype = C.c_int
    lib.hhmm_draw_stats_gauss_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_draw_stats_gauss_device.restype = C.c_int
    lib.hhmm_draw_stats_gauss.argtypes = [RP, EP]
    lib.hhmm_draw_stats_gauss.restype = C.c_int
    # include/hhmm_expect.h (the result struct is the E-step's)
    lib.hhmm_expected_stats_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_expected_stats_workspace_size.restype = C.c_int
    lib.hhmm_expected_stats_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_expected_stats_device.restype = C.c_int
    lib.hhmm_expected_stats.argtypes = [RP, EP]
    lib.hhmm_expected_stats.restype = C.c_int
    lib.hhmm_expected_stats_scan_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_expected_stats_scan_workspace_size.restype = C.c_int
    lib.hhmm_expected_stats_scan_device.argtypes = [RP, EP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_expected_stats_scan_device.restype = C.c_int
    lib.hhmm_expected_stats_scan.argtypes = [RP, EP]
    lib.hhmm_expected_stats_scan.restype = C.c_int
    # include/hhmm_estep_io.h
    IP = C.POINTER(EstepIoResult)
    lib.hhmm_estep_io_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_estep_io_workspace_size.restype = C.c_int
    lib.hhmm_estep_io_device.argtypes = [RP, IP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_estep_io_device.restype = C.c_int
    lib.hhmm_estep_io.argtypes = [RP, IP]
    lib.hhmm_estep_io.restype = C.c_int
    # include/hhmm_pointwise.h
    WP = C.POINTER(PointwiseResult)
    lib.hhmm_pointwise_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_pointwise_workspace_size.restype = C.c_int
    lib.hhmm_pointwise_device.argtypes = [RP, WP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_pointwise_device.restype = C.c_int
    lib.hhmm_pointwise.argtypes = [RP, WP]
    lib.hhmm_pointwise.restype = C.c_int
    lib.hhmm_pointwise_large_workspace_size.argtypes = [RP, C.POINTER(C.c_size_t)]
    lib.hhmm_pointwise_large_workspace_size.restype = C.c_int
    lib.hhmm_pointwise_large_device.argtypes = [RP, WP, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.hhmm_pointwise_large_device.restype = C.c_int
    lib.hhmm_pointwise_large.argtypes = [RP, WP]
    lib.hhmm_pointwise_large.restype = C.c_int
    # include/hhmm_psis.h
    if hasattr(lib, "hhmm_psis_loo"):  # absent from libraries built before PSIS (A/B variants)
        XP = C.POINTER(PsisResult)
        for kind in ("loo", "lfo"):
            getattr(lib, f"hhmm_psis_{kind}_workspace_size").argtypes = [RP, C.POINTER(C.c_size_t)]
            getattr(lib, f"hhmm_psis_{kind}_workspace_size").restype = C.c_int
            getattr(lib, f"hhmm_psis_{kind}_device").argtypes = [RP, XP, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, f"hhmm_psis_{kind}_device").restype = C.c_int
            getattr(lib, f"hhmm_psis_{kind}").argtypes = [RP, XP]
            getattr(lib, f"hhmm_psis_{kind}").restype = C.c_int
        CP = C.POINTER(PsisCellsRequest)
        lib.hhmm_psis_cells_workspace_size.argtypes = [CP, C.POINTER(C.c_size_t)]
        lib.hhmm_psis_cells_workspace_size.restype = C.c_int
        lib.hhmm_psis_cells_device.argtypes = [CP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]
        lib.hhmm_psis_cells_device.restype = C.c_int
        lib.hhmm_psis_cells.argtypes = [CP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.hhmm_psis_cells.restype = C.c_int
    return lib
