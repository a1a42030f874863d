"""ctypes binding of libdifferender_hip.so (C ABI: include/differender_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIFFERENDER_HIP_LIB lets tools/ab.sh time two builds of the library in one job (A/B on the same device). A what-if build
# (kernels that compute wrong results on purpose, csrc/dr_experiment.h) is refused unless DIFFERENDER_ALLOW_EXPERIMENT=1.
LIB_PATH = os.environ.get("DIFFERENDER_HIP_LIB") or os.path.join(_HERE, "libdifferender_hip.so")

ABI_VERSION = 9
BUILD_WRONG_RESULTS, BUILD_DIAGNOSTIC = 1, 2   # dr_build_flags()
DR_F32, DR_F16 = 0, 1
DR_MODE_DIFF, DR_MODE_NONDIFF = 0, 1
DR_VARIANT_AUTO, DR_VARIANT_BASELINE = 0, 1
DR_HINT_NO_EARLY_TERMINATION, DR_HINT_EARLY_TERMINATION = 0x100, 0x200   # OR-ed into `variant` of dr_march_fwd[_rows]
DR_COUNT_EVALUATED = 0x400   # ... and of dr_march_bwd[_rows]: measurement only (workspace header words 58-63)
DR_TAPE_TF = 0x800           # forward (DIFF) + the TF-only backward of the same inputs: per-sample tape of (intensity, lighting)
DR_SSIM_NONNEGATIVE = 1      # flags of dr_dssim_mse_fwd / _bwd: relu on the per-plane SSIM
DR_MSSSIM_MAX_LEVELS = 5     # levels of dr_msssim_mse_fwd / _bwd
DR_TV_L1, DR_TV_ISO, DR_TV_SQ = 0, 1, 2   # norm of dr_tv3d_fwd / _bwd
DR_PROJ_SUM, DR_PROJ_MAX = 0, 1           # mode of dr_project_fwd / _bwd / _bwd_cam

_c = ctypes
_P, _I, _L, _F, _D, _U, _Z = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_float, _c.c_double, _c.c_uint32, _c.c_size_t

# name -> (restype, argtypes); must list every symbol the header declares (tests/test_abi.py checks)
SIGNATURES = {
    "dr_abi_version": (_I, []),
    "dr_build_flags": (_I, []),
    "dr_error_string": (_c.c_char_p, [_I]),
    "dr_ray_setup": (_I, [_P, _I, _I, _I, _I, _I, _I, _D, _D, _F, _U, _U, _P, _P, _P, _P, _P]),
    "dr_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I]),
    "dr_workspace_bytes_tape": (_Z, [_I, _I, _I, _I, _I, _I, _I, _I, _F]),
    "dr_march_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                          _I, _I, _I, _I, _F, _D, _D, _I, _I, _P, _P, _P, _Z, _P]),
    "dr_march_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                          _I, _I, _I, _I, _F, _D, _D, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P, _Z, _P]),
    "dr_ray_setup_rows": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _D, _D, _F, _U, _U, _P, _P, _P, _P, _P]),
    "dr_march_fwd_rows": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _D, _D, _I, _I, _P, _P, _P, _Z, _I, _I, _P]),
    "dr_march_bwd_rows": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _D, _D, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P, _Z, _I, _I, _P]),
    "dr_march_bwd_cam": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                              _I, _I, _I, _I, _F, _D, _D, _U, _U, _I, _I, _P, _P, _P, _P, _P, _P]),
    # the free camera: the entries above plus pose, fov_v (and d_pose, d_pose_ray for d_cam, d_cam_ray)
    "dr_ray_setup_pose_rows": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _D, _D, _F, _U, _U, _P, _P, _P, _P, _P, _P, _P]),
    "dr_march_fwd_rows_pose": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                                    _I, _I, _I, _I, _F, _D, _D, _I, _I, _P, _P, _P, _Z, _I, _I, _P, _P, _P]),
    "dr_march_bwd_rows_pose": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                                    _I, _I, _I, _I, _F, _D, _D, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P, _Z, _I, _I, _P, _P, _P]),
    "dr_march_bwd_pose": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _D, _D, _U, _U, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dr_project_bwd_pose": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _D, _D, _U, _U,
                                 _P, _P, _P, _P, _P, _P, _P]),
    "dr_march_bwd_variant": (_I, [_I, _I, _I, _I, _I, _I, _I, _L, _L, _L, _L, _L, _L, _I, _I, _I]),
    "dr_comm_unique_id": (_I, [_P]),
    "dr_comm_init_rank": (_I, [_c.POINTER(_P), _I, _P, _I]),
    "dr_comm_init_all": (_I, [_c.POINTER(_P), _I, _c.POINTER(_I)]),
    "dr_allreduce_f32": (_I, [_P, _P, _Z, _P]),
    "dr_allreduce_gradients_f32": (_I, [_P, _P, _Z, _P, _Z, _P]),
    "dr_comm_destroy": (_I, [_P]),
    "dr_mse_loss_grad": (_I, [_P, _P, _L, _F, _P, _P, _P]),
    "dr_tf_momentum_step": (_I, [_P, _P, _P, _I, _F, _F, _F, _P]),
    "dr_dssim_mse_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _D, _I, _D, _D, _D, _I, _P, _P]),
    "dr_dssim_mse_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _D, _I, _D, _D, _D, _I, _P, _P, _P, _P, _P]),
    "dr_msssim_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "dr_msssim_mse_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _D, _I, _D, _D, _D, _P, _I, _P, _P, _P]),
    "dr_msssim_mse_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _D, _I, _D, _D, _D, _P, _I, _P, _P, _P, _P, _P, _P]),
    "dr_tv3d_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _D, _P, _P]),
    "dr_tv3d_bwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _D, _P, _F, _P, _P, _I, _P]),
    "dr_march_tf2d_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _I, _L, _F, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _I, _P, _P, _P]),
    "dr_march_tf2d_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _I, _L, _F, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P]),
    "dr_march_rgba_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _L, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _I, _P, _P, _P]),
    "dr_march_rgba_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _L, _P, _P, _P, _P, _P,
                               _I, _I, _I, _I, _F, _P, _P, _P, _L, _L, _L, _L, _L, _P]),
    "dr_march_rgba_bwd_cam": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _L, _P, _P, _P, _P, _P,
                                   _I, _I, _I, _I, _F, _D, _D, _U, _U, _P, _P, _P, _P, _P, _P]),
    "dr_march_rgba_bwd_pose": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _L, _P, _P, _P, _P, _P,
                                    _I, _I, _I, _I, _F, _D, _D, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P]),
    # the lit march: dr_march_fwd / _bwd in their plain form plus light, mode (and d_light, d_light_ray)
    "dr_march_lit_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                              _I, _I, _I, _I, _F, _P, _I, _P, _P, _P]),
    "dr_march_lit_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                              _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P, _P, _P]),
    # the depth moments: dr_march_fwd's volume, TF and ray arguments, then out, steps / the backward's
    # gradients / the tails of dr_march_rgba_bwd_cam / _bwd_pose
    "dr_march_depth_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                                _I, _I, _I, _I, _F, _P, _P, _P]),
    "dr_march_depth_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                                _I, _I, _I, _I, _F, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P]),
    "dr_march_depth_bwd_cam": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                                    _I, _I, _I, _I, _F, _D, _D, _U, _U, _P, _P, _P, _P, _P, _P]),
    "dr_march_depth_bwd_pose": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _I, _L, _P, _P, _P, _P, _P,
                                     _I, _I, _I, _I, _F, _D, _D, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P]),
    # the ray bundle: origins, dirs and N in the camera's and the image's place; one volume, one table
    "dr_bundle_setup": (_I, [_P, _P, _L, _I, _I, _I, _F, _F, _U, _U, _P, _P, _P, _P]),
    "dr_march_bundle_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P]),
    "dr_march_bundle_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P,
                                 _P, _L, _L, _L, _P, _P]),
    "dr_march_bundle_bwd_rays": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F,
                                      _P, _F, _U, _U, _P, _P, _P, _P, _P]),
    # the projections of a ray bundle: the bundle's arguments without the table, mode and arg_max
    "dr_project_bundle_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P]),
    "dr_project_bundle_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _P, _P, _P, _P, _L, _I, _I, _P, _P,
                                   _P, _L, _L, _L, _I, _P]),
    "dr_project_bundle_bwd_rays": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _P, _P, _P, _P, _L, _I, _I, _F, _U, _U,
                                        _P, _P, _P, _P, _P]),
    # the RGBA march of a ray bundle: the bundle's arguments with the RGBA volume's (sc, dsc) in the table's place
    "dr_march_rgba_bundle_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P]),
    "dr_march_rgba_bundle_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P,
                                      _P, _L, _L, _L, _L, _P]),
    "dr_march_rgba_bundle_bwd_rays": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _L, _I, _F,
                                           _P, _F, _U, _U, _P, _P, _P, _P, _P]),
    # the depth moments of a ray bundle: exactly the argument lists of the D19 entries
    "dr_march_depth_bundle_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P]),
    "dr_march_depth_bundle_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P,
                                       _P, _L, _L, _L, _P, _P]),
    "dr_march_depth_bundle_bwd_rays": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F,
                                            _P, _F, _U, _U, _P, _P, _P, _P, _P]),
    "dr_project_fwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dr_project_bwd": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P,
                            _P, _L, _L, _L, _L, _I, _P]),
    "dr_project_bwd_cam": (_I, [_P, _I, _I, _I, _I, _L, _L, _L, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _D, _D, _U, _U,
                                _P, _P, _P, _P, _P]),
}

_lib = None


def lib():
    """Load the HIP library (once). Raises ImportError with a build hint if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C differender_amd/csrc`). differender_amd has no CPU or PyTorch fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        rebuild = "rebuild it (`make -C differender_amd/csrc`), or unset DIFFERENDER_HIP_LIB"
        # the version FIRST: a stale library lacks newer symbols, and the loop over SIGNATURES below would die on the first of
        # them with a bare AttributeError before the "ABI version ..., rebuild it" hint was ever reached
        try:
            handle.dr_abi_version.restype = ctypes.c_int
            version = handle.dr_abi_version()
        except AttributeError as exc:
            raise ImportError(f"{LIB_PATH} does not export dr_abi_version: not this package's library; {rebuild}") from exc
        # (same-device A/B against the library of an EARLIER round -- tools/abn.sh with ab_libs/r05.so: DIFFERENDER_AB_OLD_ABI=8 accepts
        #  that one older version; entry points it lacks are simply absent, and whatever needs them fails when it is called)
        ab_old = os.environ.get("DIFFERENDER_AB_OLD_ABI") == str(abs(version)) and abs(version) < ABI_VERSION
        if abs(version) != ABI_VERSION and not ab_old:
            raise ImportError(f"{LIB_PATH}: ABI version {version}, expected {ABI_VERSION}; {rebuild}")
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as exc:
                if ab_old:
                    continue
                raise ImportError(f"{LIB_PATH} reports ABI version {version} but does not export `{name}`; {rebuild}") from exc
            fn.restype = res
            fn.argtypes = args
        flags = handle.dr_build_flags()
        if (version < 0 or flags & BUILD_WRONG_RESULTS) and os.environ.get("DIFFERENDER_ALLOW_EXPERIMENT") != "1":
            raise ImportError(
                f"{LIB_PATH} is a what-if build whose kernels compute WRONG results on purpose (dr_build_flags() = {flags}); "
                "it is for timing experiments only. Set DIFFERENDER_ALLOW_EXPERIMENT=1 to load it anyway.")
        if flags & BUILD_WRONG_RESULTS:
            import warnings
            warnings.warn(f"{LIB_PATH}: what-if build, results are WRONG by construction", RuntimeWarning)
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().dr_error_string(code)
        raise RuntimeError(f"{what} failed: {msg.decode() if msg else code} (code {code})")
