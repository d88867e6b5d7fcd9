"""The C-ABI library loads (no GPU needed) and exports exactly what include/partmanip_hip.h
declares; the ctypes table in partmanip_amd/_lib.py matches the header's parameter counts."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "partmanip_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(pm_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        out[m.group(2)] = (m.group(1), n)
    return out


def test_header_declares_the_survey_minimum_symbol_set():
    fns = header_functions()
    # SURVEY.md 8(b)'s list, name for name ...
    for need in ("pm_gae_scan_f32", "pm_adv_normalize_f32", "pm_gather_rows_f32", "pm_mlp_fwd_f32", "pm_mlp_bwd_f32",
                 "pm_pointnet_enc_fwd_f32", "pm_pointnet_enc_bwd_f32", "pm_ppo_actor_loss_fwd_bwd_f32", "pm_value_loss_fwd_bwd_f32",
                 "pm_mse_tanh_loss_fwd_bwd_f32", "pm_clip_adam_step_f32", "pm_fps_f32", "pm_ball_query_f32", "pm_group_points_f32",
                 "pm_group_points_bwd_f32", "pm_version"):
        assert need in fns, need
    # ... and the finer-grained forms the learner itself calls (INTEGRATION.md maps one to the other)
    for need in ("pm_gae_scan_f32", "pm_gather_rows_f32", "pm_linear_fwd_f32", "pm_linear_bwd_data_f32", "pm_moments_f64",
                 "pm_normalize_apply_f32",
                 "pm_linear_bwd_weight_f32", "pm_pointnet_enc_fwd_f32", "pm_pointnet_enc_bwd_f32",
                 "pm_ppo_actor_loss_fwd_bwd_f32", "pm_value_loss_fwd_bwd_f32", "pm_mse_tanh_loss_fwd_bwd_f32",
                 "pm_clip_adam_step_f32", "pm_fps_f32", "pm_ball_query_f32", "pm_group_points_f32",
                 "pm_group_points_bwd_f32", "pm_version",
                 "pm_sparse_conv_fwd_variant_f32", "pm_sparse_conv_bwd_data_variant_f32",
                 "pm_sparse_conv_bwd_data_scatter_variant_f32", "pm_sparse_conv_bwd_weight_variant_f32"):
        assert need in fns, need


def test_library_exports_every_declared_symbol_and_ctypes_table_matches():
    from partmanip_amd import _lib
    fns = header_functions()
    assert len(fns) >= 25
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, nargs) in fns.items():
        assert hasattr(so, name), f"{name} declared in the header but missing from the .so"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes binding"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs, f"{name}: header has {nargs} parameters, ctypes table {len(args)}"
        assert (res is ctypes.c_size_t) == (ret == "size_t"), name
    assert set(_lib.SIGNATURES) == set(fns)
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "partmanip_hip.h")).read()
    want = int(re.search(r"#define PM_ABI_VERSION (\d+)", hdr).group(1))
    from partmanip_amd import _lib
    assert so.pm_version() == want == _lib.ABI_VERSION


def test_ctypes_table_matches_the_header_parameter_types_position_by_position():
    """Round 6: a binding with the right NUMBER of parameters but an int where the header has a pointer (one slot off) is a memory
    fault on the GPU box, not an error here -- so every position's C type is compared with its ctypes class: any `*` -> c_void_p,
    int -> c_int, long -> c_long, size_t -> c_size_t, float -> c_float, double -> c_double, unsigned -> c_uint."""
    from partmanip_amd import _lib
    src = open(os.path.join(ROOT, "include", "partmanip_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
             "unsigned": ctypes.c_uint, "int32_t": ctypes.c_int, "uint32_t": ctypes.c_uint}
    checked = 0
    for m in re.finditer(r"\b(int|size_t)\s+(pm_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        name, args = m.group(2), m.group(3).strip()
        if args in ("", "void"):
            continue
        want = []
        for a in args.split(","):
            a = a.strip()
            if "*" in a:
                want.append(ctypes.c_void_p)
            else:
                toks = [t_ for t_ in a.replace("const", " ").split() if t_]
                want.append(kinds[toks[0]])
        got = _lib.SIGNATURES[name][1]
        assert len(got) == len(want), name
        for i, (g_, w_) in enumerate(zip(got, want)):
            assert g_ is w_, f"{name}: parameter {i} is {w_.__name__} in the header, {g_.__name__} in the ctypes table"
            checked += 1
    assert checked > 1000


def test_argument_validation_without_gpu():
    """Null pointers / bad sizes are rejected before any launch (safe on a GPU-less host)."""
    from partmanip_amd._lib import lib
    assert lib.pm_gae_scan_f32(None, None, None, None, None, None, None, 4, 4, 0.99, 0.94, 0, 0.0, None) == -1
    assert lib.pm_linear_fwd_f32(None, 0, None, 0, None, None, 0, 1, 1, 1, 0, None) == -1
    assert lib.pm_pointnet_enc_fwd_f32(None, 0, 1, 1000, 3, 0, None, None, None, None, None, 1, None, 0, None, None, 1, None) == -1
    assert lib.pm_pointnet_packed_elems() == 196608 + 32768 + 1024      # fwd W2|W3, bwd W2^T in two MFMA operand orders, pad
    assert lib.pm_moments_workspace_bytes(10) >= 16
    # the split-bf16 backward: no packed planes / no saved layer 2 -> refused (never a silent fp32 run)
    assert lib.pm_pointnet_enc_bwd_bf6(None, 0, 1, 1024, 3, 0, None, None, None, None, None, None, 1, None, 0, None, None, None,
                                       None, None, None, None, None, None, 0, None) == -1
    assert lib.pm_pointnet_packed_bwd_bf6_bytes() == (3 * 4 * 16 * 64 * 8 + 4096) * 2
    assert lib.pm_fps_varlen_workspace_bytes(4, 8192) == 0
    assert lib.pm_fps_varlen_workspace_bytes(4, 10000) == 160000 + (2 * 256 * 8 + 1) * 8    # two sets x 256 work-groups x 8 words + the error word
    assert lib.pm_fps_workspace_bytes(2, 1024) == 0 and lib.pm_fps_workspace_bytes(2, 20000) == 160000


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from partmanip_amd import ops
    x = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_fwd(x, x, x[0], x, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gae_scan(x, x, x, x, x, x, x, 0.9, 0.9, None)
