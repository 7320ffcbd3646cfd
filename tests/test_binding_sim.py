"""The typed pointer arguments of the C ABI binding (ccd_amd/_lib.py) on the CPU SIMT executor's library.  No kernel runs: a rejected
argument never reaches the library, and the accepted ones go to calls that return CCD_EINVAL / CCD_ESHAPE before any launch."""
import ctypes

import pytest
import torch

from backends import Backend

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_wrong_dtype_is_a_type_error_naming_entry_point_and_parameter(sim):
    from ccd_amd import _lib, ops
    a, b = torch.zeros((8, 64), dtype=BF16), torch.zeros((8, 64), dtype=BF16)
    with pytest.raises(TypeError, match=r"^ccd_gemm_nt: bias expects float32, got bfloat16$"):
        ops.gemm_nt(a, b, bias=torch.zeros(8, dtype=BF16))
    with pytest.raises(TypeError, match=r"^ccd_gemm_nt: A expects bfloat16, got float32$"):
        ops.gemm_nt(a.float(), b)
    x, w = torch.zeros((4, 64)), torch.ones(64)
    with pytest.raises(TypeError, match=r"^ccd_ln_fwd: x expects float32, got bfloat16$"):
        ops.ln_fwd(x.bfloat16(), w, w)
    with pytest.raises(TypeError, match=r"^ccd_ln_fwd: gamma expects float32, got float64$"):
        ops.ln_fwd(x, w.double(), w)
    # wrappers that never checked a dtype themselves: the DINO head, the optimizer tables, the datapipe
    with pytest.raises(TypeError, match=r"^ccd_l2norm_fwd: x expects bfloat16, got float32$"):
        ops.l2norm_fwd(x, x.bfloat16(), torch.zeros(4))
    i32, i64, t = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(64)
    with pytest.raises(TypeError, match=r"^ccd_seg_sumsq: chunk_begin expects int64, got int32$"):
        ops.seg_sumsq(t, i32, i32, i32, t)
    with pytest.raises(TypeError, match=r"^ccd_seg_sumsq: chunk_seg expects int32, got int64$"):
        ops.seg_sumsq(t, i64, i64, i32, t)
    with pytest.raises(TypeError, match=r"^ccd_droppath_scales: d_seed expects int64 or uint64, got int32$"):
        ops.droppath_scales(torch.ones(2), 4, 1, d_seed=i32)
    with pytest.raises(TypeError, match=r"^ccd_region_stats: idmap expects uint8, got float32$"):
        ops.region_stats(torch.zeros((2, 32, 128)))
    # called past the wrappers, the library itself refuses the tensor (ctypes' own error type)
    with pytest.raises(ctypes.ArgumentError, match=r"argument 1: TypeError: expects float32, got bfloat16"):
        _lib.get().ccd_ln_fwd(x.bfloat16(), w, w, x.bfloat16(), w, w, 4, 64, 1e-6, 0)


def test_strided_innermost_dimension_is_a_value_error(sim):
    from ccd_amd import ops
    w = torch.ones(64)
    with pytest.raises(ValueError, match=r"^ccd_ln_fwd: x innermost dimension must be contiguous$"):
        ops.ln_fwd(torch.zeros((64, 4)).t(), w, w)
    with pytest.raises(ValueError, match=r"^ccd_ln_fwd: beta innermost dimension must be contiguous$"):
        ops.ln_fwd(torch.zeros((4, 64)), w, torch.ones(128)[::2])
    with pytest.raises(ValueError, match=r"^ccd_gemm_nt: C2 innermost dimension must be contiguous$"):     # behind a void*, too
        ops.gemm_nt(torch.zeros((8, 64), dtype=BF16), torch.zeros((8, 64), dtype=BF16), epilogue=ops.EPI_GELU,
                    out2=torch.zeros((8, 8), dtype=BF16).t())


def test_none_int_and_ctypes_values_pass_a_typed_pointer(sim):
    from ccd_amd import _lib
    lib = _lib.get()
    t, i32, i64 = torch.zeros(64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    host = (ctypes.c_float * 64)()
    # ccd_seg_moments: CCD_EINVAL for a missing pointer or an empty chunk table, before any launch
    assert lib.ccd_seg_moments(t, None, i32, i64, i32, 1, t, 0) == -1                                   # tensors and None
    assert lib.ccd_seg_moments(t, t, i32, i64, i32, 0, t, None) == -1                                   # (the stream, too)
    assert lib.ccd_seg_moments(t.data_ptr(), t.data_ptr(), i32.data_ptr(), i64.data_ptr(), i32.data_ptr(), 0, t.data_ptr(), 0) == -1
    assert lib.ccd_seg_moments(host, ctypes.cast(host, ctypes.POINTER(ctypes.c_float)), i32, i64, i32, 0, ctypes.c_void_p(t.data_ptr()),
                               0) == -1
    v = ctypes.c_int(-7)
    assert lib.ccd_policy_get(b"rowgemm", ctypes.byref(v)) == 0 and v.value in (0, 1, 2)
    assert lib.ccd_policy_get(b"no_such_key", ctypes.byref(v)) == -1
    # an address above 2^32 arrives whole
    assert "0x10000000010" in repr(_lib.SIGNATURES["ccd_permute4"][1].from_param((1 << 40) + 16))        # <cparam 'P' (0x...)>
    assert _lib.SIGNATURES["ccd_ln_fwd"][0].from_param(t).value == t.data_ptr()
    with pytest.raises(ctypes.ArgumentError):
        lib.ccd_seg_moments(1.5, t, i32, i64, i32, 0, t, 0)


def test_structure_goes_by_reference(sim):
    from ccd_amd import _lib, ops
    desc = ops.conv_desc((2, 2), (2, 2), 8, [(0, 0)])
    assert _lib.SIGNATURES["ccd_conv_gemm"][2].from_param(desc)._obj is desc            # ctypes.byref(desc)


def test_void_pointer_takes_either_float_format(sim):
    from ccd_amd import _lib
    lib = _lib.get()
    for dt in (F32, BF16):
        src = torch.zeros(8, dtype=dt)
        # n % 4 != 0: CCD_ESHAPE before any launch
        assert lib.ccd_dropout(src, int(dt == BF16), None, src, int(dt == BF16), 6, 1, 0.5, 0) == -2, dt
    assert _lib.SIGNATURES["ccd_dropout"][0].dtypes is None and _lib.SIGNATURES["ccd_dropout"][2].dtypes == (F32,)
