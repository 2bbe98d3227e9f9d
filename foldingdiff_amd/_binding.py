"""
ctypes binding of libfdmi.so (C ABI declared in include/fdmi.h).

There is deliberately no fallback: if the shared library is missing or the call
fails, a RuntimeError / FdmiError is raised.  The product path never computes on
the CPU.
"""
import ctypes as C
import os
from typing import Optional

LIB_PATH = os.environ.get("FDMI_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libfdmi.so")  # FDMI_LIB: A/B builds

FD_OK = 0
FD_POS = {"absolute": 0, "relative_key": 1, "relative_key_query": 2}
FD_DEC = {"mlp": 0, "linear": 1}
FD_PREC_F32 = 0
FD_PREC_F16X3 = 1
FD_PREC = {"f32": 0, "f16x3": 1}
ABI_VERSION = 7


class FdmiError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libfdmi error {code}: {msg}")
        self.code = code


class FdConfig(C.Structure):
    _fields_ = [
        ("n_features", C.c_int32),
        ("d_model", C.c_int32),
        ("n_heads", C.c_int32),
        ("d_ff", C.c_int32),
        ("n_layers", C.c_int32),
        ("max_pos", C.c_int32),
        ("pos_type", C.c_int32),
        ("decoder", C.c_int32),
        ("ln_eps", C.c_float),
    ]


class FdSteerParams(C.Structure):
    """``fd_steer_params`` of include/fdmi.h."""
    _fields_ = [
        ("weights", C.c_double * 4),
        ("lam", C.c_double),
        ("ess_frac", C.c_double),
        ("clash_alpha", C.c_double),
        ("feat_idx", C.c_int32 * 9),
        ("has_offset", C.c_int32),
        ("offset", C.c_float * 16),
    ]


class FdGuideParams(C.Structure):
    """``fd_guide_params`` of include/fdmi.h."""
    _fields_ = [
        ("feat_idx", C.c_int32 * 9),
        ("has_offset", C.c_int32),
        ("offset", C.c_float * 16),
        ("max_norm", C.c_double),
    ]


class FdScaffoldGuideParams(C.Structure):
    """``fd_scaffold_guide_params`` of include/fdmi.h."""
    _fields_ = [
        ("feat_idx", C.c_int32 * 9),
        ("has_offset", C.c_int32),
        ("offset", C.c_float * 16),
        ("max_norm", C.c_double),
        ("clash_alpha", C.c_double),
        ("clash_margin", C.c_double),
        ("w_clash", C.c_double),
    ]


class FdRelaxParams(C.Structure):
    """``fd_relax_params`` of include/fdmi.h."""
    _fields_ = [
        ("feat_idx", C.c_int32 * 9),
        ("is_angle", C.c_uint8 * 16),
        ("move", C.c_uint8 * 16),
        ("clash_alpha", C.c_double),
        ("clash_margin", C.c_double),
        ("w_clash", C.c_double),
        ("w_tether", C.c_double),
        ("step0", C.c_double),
        ("grow", C.c_double),
        ("shrink", C.c_double),
        ("max_step", C.c_double),
    ]


class FdSymmetryParams(C.Structure):
    """``fd_symmetry_params`` of include/fdmi.h."""
    _fields_ = [
        ("clash_alpha", C.c_double),
        ("clash_margin", C.c_double),
        ("w_clash", C.c_double),
        ("w_contact", C.c_double),
        ("d_on", C.c_double),
        ("d_off", C.c_double),
        ("w_radial", C.c_double),
        ("r_max", C.c_double),
        ("lever", C.c_double),
        ("max_shift", C.c_double),
        ("step0", C.c_double),
        ("grow", C.c_double),
        ("shrink", C.c_double),
        ("pose_iters", C.c_int32),
        ("reserved", C.c_int32),
    ]


# every symbol include/fdmi.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_SIGNATURES = {
    "fd_abi_version": (C.c_int, []),
    "fd_device_count": (C.c_int, []),
    "fd_create": (C.c_int, [C.POINTER(FdConfig), C.c_int, C.POINTER(_P)]),
    "fd_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "fd_finalize": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "fd_destroy": (None, [_P]),
    "fd_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "fd_forward": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "fd_forward_t": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "fd_ar_forward": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "fd_ar_sample": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "fd_forward_ex": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "fd_p_sample_step": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "fd_sample": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_uint64, _P, C.c_int]),
    "fd_sample_ex": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_uint64, C.c_int64, _P, C.c_int]),
    "fd_sample_inpaint": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P, C.c_int]),
    "fd_p_sample_step_inpaint": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P]),
    "fd_sample_inpaint_resample": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, C.c_uint64, C.c_int64, _P]),
    "fd_inpaint_jump": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P, C.c_uint64, C.c_int64, _P]),
    "fd_sample_strided": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.c_int64, _P, C.c_int]),
    "fd_sample_strided_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.c_int64, _P, C.c_int, _P]),
    "fd_p_sample_step_coef": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P, C.c_int, _P, _P]),
    "fd_sample_strided_inpaint": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P,
                                            C.c_int]),
    "fd_sample_strided_inpaint_resample": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P,
                                                     C.c_uint64, C.c_int64, _P]),
    "fd_p_sample_step_coef_inpaint": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P, C.c_int,
                                                C.c_int, _P, _P, _P, _P, _P, _P]),
    "fd_sample_solver": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int]),
    "fd_sample_solver_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, _P]),
    "fd_p_sample_step_solver": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                          _P, C.c_int, _P, _P, _P]),
    "fd_sample_steered": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.c_int64, _P, C.c_int,
                                    C.POINTER(FdSteerParams), _P, _P, _P, _P, _P, _P]),
    "fd_p_sample_step_coef_x0": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                           _P, C.c_int, _P, _P, _P]),
    "fd_steer_rewards": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, _P, _P]),
    "fd_steer_resample": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P, _P]),
    "fd_sample_repeat": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.c_int64, _P, _P]),
    "fd_tie_repeats": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, _P, C.c_uint64, C.c_int, C.c_int64,
                                 _P]),
    "fd_nerf_vjp": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "fd_nerf_vjp_feats": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "fd_restraint_energy": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_guide_step": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_double,
                                C.c_float, _P, C.c_uint64, C.c_int, C.c_int64, _P, _P, _P]),
    "fd_sample_guided": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.c_int64, _P, C.POINTER(FdGuideParams),
                                   _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_scaffold_guide_step": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(FdScaffoldGuideParams), _P, _P, _P,
                                         _P, _P, _P, C.c_float, C.c_float, _P, C.c_uint64, C.c_int, C.c_int64, _P, _P, _P, _P, _P]),
    "fd_sample_guided_inpaint": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P,
                                           C.POINTER(FdScaffoldGuideParams), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_template_energy": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_scaffold_guide_step_tpl": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(FdScaffoldGuideParams), _P, _P,
                                             _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, _P, C.c_uint64, C.c_int, C.c_int64, _P, _P, _P,
                                             _P, _P, _P]),
    "fd_sample_guided_inpaint_tpl": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P,
                                               C.POINTER(FdScaffoldGuideParams), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_symmetry_energy": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(FdSymmetryParams), _P, _P, _P, _P]),
    "fd_symmetry_dock": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(FdSymmetryParams), C.c_int, _P, _P, _P, _P, _P, _P]),
    "fd_scaffold_guide_step_sym": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(FdScaffoldGuideParams), _P, _P,
                                             _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(FdSymmetryParams), _P, C.c_float, C.c_float,
                                             _P, C.c_uint64, C.c_int, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_sample_guided_inpaint_sym": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P,
                                               C.POINTER(FdScaffoldGuideParams), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                               C.POINTER(FdSymmetryParams), _P, _P, _P, _P, _P, _P, _P]),
    "fd_nerf_scan": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "fd_relax_energy": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(FdRelaxParams), _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                  _P]),
    "fd_relax": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(FdRelaxParams), _P, _P, _P, _P, _P, _P, _P, C.c_int, _P,
                           _P, _P, _P, _P]),
    "fd_sample_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_uint64, C.c_int64, _P, C.c_int, _P]),
    "fd_sample_begin_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int64, _P, C.c_int, _P]),
    "fd_sample_steps_dev": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "fd_sample_end_dev": (C.c_int, [_P, _P, _P]),
    "fd_comm_unique_id": (C.c_int, [_P]),
    "fd_comm_init": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "fd_gather_dev": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "fd_comm_destroy": (C.c_int, [_P]),
    "fd_philox_normal_dev": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_int64, C.c_int, C.c_int, _P, _P]),
    "fd_nerf": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "fd_internal_coords": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, _P]),
    "fd_superpose_rmsd": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "fd_tm_score": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "fd_annotate_sse": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, _P, _P]),
    "fd_backbone_oxygens": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]),
    "fd_dssp": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "fd_tm_align": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "fd_tm_align_ex": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_uint32, _P]),
    "fd_backbone_clashes": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_double, _P, _P]),
    "fd_lddt": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_double, _P, C.c_int, _P, _P]),
    "fd_loss_terms": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, _P, _P]),
    "fd_denoise_loss": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P]),
    "fd_loss_terms_ex": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P]),
    "fd_pairwise_dist": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "fd_denoise_loss_ex": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P,
                                     _P, _P, _P, _P]),
    "fd_hist_columns": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int, _P, C.c_int, _P, _P, _P]),
    "fd_noise_minmax": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_uint64, C.c_uint64,
                                  C.c_int64, _P, _P, _P]),
    "fd_noise_hist": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_uint64, C.c_uint64,
                                C.c_int64, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "fd_shift_trim_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "fd_test_wrap": (C.c_int, [C.c_int, C.c_int, _P, C.c_int64, _P]),
    "fd_test_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "fd_test_gemm_ln": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_int, C.c_int, C.c_int]),
    "fd_test_gemm_time": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "fd_profile_every": (C.c_int, [_P, C.c_int]),
    "fd_profile_reset": (C.c_int, [_P]),
    "fd_profile_count": (C.c_int, [_P]),
    "fd_profile_get": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fd_synchronize": (C.c_int, [_P]),
    "fd_check_finite": (C.c_int, [_P]),
    "fd_fused_attn_supported": (C.c_int, [_P, C.c_int]),
    "fd_debug_read": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "fd_last_error": (C.c_char_p, []),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen libfdmi.so and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. "
            "Run `python -m foldingdiff_amd.build` (needs hipcc). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    # the version first: an older library then fails with a version message, not with a missing-symbol AttributeError
    lib.fd_abi_version.restype = C.c_int
    lib.fd_abi_version.argtypes = []
    v = lib.fd_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: libfdmi ABI version {v}, this binding expects {ABI_VERSION}; "
                           "rebuild with `python -m foldingdiff_amd.build --force`")
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError => header / library mismatch, surface it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return list(_SIGNATURES.keys())


def ptr(a):
    """The address of a numpy array as a ``void*`` argument, ``None`` (a null pointer) for ``None``."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(rc: int):
    if rc != FD_OK:
        msg = load().fd_last_error()
        raise FdmiError(rc, msg.decode("utf-8", "replace") if msg else "")
