"""The two helpers behind the device-memory methods of BatchedLexLSE (lexls_amd/lexlse.py) — _device_address, the address of an optional device
argument, and _leading_axis, the optional leading axis K of solve_tangent(_device) and solve_rhs(_device) — on CPU torch tensors: no device is
touched, the helpers only look at a tensor's dtype, strides, shape and data_ptr().  The ValueError texts are the ones the five methods raised
when each had a closure of its own."""
import ctypes as C

import pytest
import torch

from lexls_amd.lexlse import _device_address, _leading_axis

F64, U8 = "torch.float64", "torch.uint8"


def test_none_stays_none_whatever_else_is_asked():
    for raw_ok in (False, True):
        assert _device_address("solve_adjoint_device", "grad_fixed", None, (2, 3), raw_ok=raw_ok) is None
        assert _device_address("solve_tangent_device", "differentiable", None, (2,), U8, raw_ok=raw_ok) is None


def test_a_tensor_of_the_dtype_and_shape_gives_its_address():
    t = torch.zeros((2, 3), dtype=torch.float64)
    flags = torch.zeros(2, dtype=torch.uint8)
    for raw_ok in (False, True):
        a = _device_address("solve_adjoint_device", "g", t, (2, 3), raw_ok=raw_ok)
        assert isinstance(a, C.c_void_p) and a.value == t.data_ptr()
        a = _device_address("solve_adjoint_matrix_device", "differentiable", flags, (2,), U8, raw_ok=raw_ok)
        assert isinstance(a, C.c_void_p) and a.value == flags.data_ptr()


def test_a_raw_address_is_taken_where_the_method_accepts_one():
    """solve_adjoint_device and solve_adjoint_matrix_device (raw_ok) take an integer as it is, dtype and shape unchecked"""
    a = _device_address("solve_adjoint_device", "g", 0x7f0000001000, (2, 3), raw_ok=True)
    assert isinstance(a, C.c_void_p) and a.value == 0x7f0000001000
    a = _device_address("solve_adjoint_matrix_device", "differentiable", 4096, (2,), U8, raw_ok=True)
    assert isinstance(a, C.c_void_p) and a.value == 4096


@pytest.mark.parametrize("who, text", [
    ("solve_adjoint_multi_device", "solve_adjoint_multi_device: G must be a contiguous float64 tensor of shape (2, 5, 3)"),
    ("solve_tangent_device", "solve_tangent_device: G must be a contiguous float64 tensor of shape (2, 5, 3)"),
    ("solve_rhs_device", "solve_rhs_device: G must be a contiguous float64 tensor of shape (2, 5, 3)"),
])
def test_a_raw_address_is_refused_where_the_method_accepts_none(who, text):
    with pytest.raises(ValueError) as e:
        _device_address(who, "G", 0x7f0000001000, (2, 5, 3))
    assert str(e.value) == text


WRONG = {
    "dtype": lambda: torch.zeros((2, 3), dtype=torch.float32),
    "non-contiguous": lambda: torch.zeros((3, 2), dtype=torch.float64).t(),
    "shape": lambda: torch.zeros((2, 4), dtype=torch.float64),
    "rank": lambda: torch.zeros((1, 2, 3), dtype=torch.float64),
}


@pytest.mark.parametrize("what", sorted(WRONG))
@pytest.mark.parametrize("who, raw_ok, text", [
    ("solve_adjoint_device", True, "solve_adjoint_device: g must be a contiguous float64 tensor of shape (2, 3)"),
    ("solve_adjoint_multi_device", False, "solve_adjoint_multi_device: g must be a contiguous float64 tensor of shape (2, 3)"),
    ("solve_adjoint_matrix_device", True, "solve_adjoint_matrix_device: g must be a contiguous float64 tensor of shape (2, 3)"),
    ("solve_tangent_device", False, "solve_tangent_device: g must be a contiguous float64 tensor of shape (2, 3)"),
    ("solve_rhs_device", False, "solve_rhs_device: g must be a contiguous float64 tensor of shape (2, 3)"),
])
def test_a_tensor_of_the_wrong_kind_is_refused_in_the_method_s_words(who, raw_ok, text, what):
    t = WRONG[what]()
    assert tuple(t.shape) == (2, 3) or what in ("shape", "rank")
    with pytest.raises(ValueError) as e:
        _device_address(who, "g", t, (2, 3), raw_ok=raw_ok)
    assert str(e.value) == text


@pytest.mark.parametrize("who, raw_ok, text", [
    ("solve_adjoint_matrix_device", True, "solve_adjoint_matrix_device: differentiable must be a contiguous uint8 tensor of shape (2,)"),
    ("solve_tangent_device", False, "solve_tangent_device: differentiable must be a contiguous uint8 tensor of shape (2,)"),
])
def test_the_flags_are_uint8_and_the_text_names_the_dtype_asked_for(who, raw_ok, text):
    for t in (torch.zeros(2, dtype=torch.bool), torch.zeros(2, dtype=torch.float64), torch.zeros(3, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError) as e:
            _device_address(who, "differentiable", t, (2,), U8, raw_ok=raw_ok)
        assert str(e.value) == text


def test_the_leading_axis_on_both_ranks():
    # one item without the axis: nothing stands in front of an item's shape, K = 1
    assert _leading_axis((2, 4, 3), 3) == ((), 1)   # dlod (batch, nVar + 1, cap)
    assert _leading_axis((2, 3), 2) == ((), 1)      # rhs (batch, cap)
    assert _leading_axis(torch.zeros((2, 3)).shape, 2) == ((), 1)
    # K items
    assert _leading_axis((5, 2, 4, 3), 3) == ((5,), 5)
    assert _leading_axis((1, 2, 3), 2) == ((1,), 1)  # (K = 1 given WITH the axis keeps it: the results have it too)
    lead, K = _leading_axis(torch.zeros((65, 2, 3)).shape, 2)
    assert lead == (65,) and K == 65 and type(K) is int and type(lead[0]) is int


def test_the_leading_axis_gives_k_zero_for_what_the_callers_refuse():
    assert _leading_axis((0, 2, 4, 3), 3) == ((0,), 0)  # no item
    assert _leading_axis((0, 2, 3), 2) == ((0,), 0)
    for shape, rank in (((2,), 2), ((1, 1, 2, 3), 2), ((4, 3), 3), ((1, 1, 2, 4, 3), 3), ((), 2)):  # neither rank
        assert _leading_axis(shape, rank)[1] == 0


class _Handle:
    """what the four methods read of a BatchedLexLSE before they reach the library"""
    batch, nVar, cap, _h = 2, 3, 3, None


def _refusal(method, *args):
    from lexls_amd import BatchedLexLSE
    with pytest.raises(ValueError) as e:
        getattr(BatchedLexLSE, method)(_Handle(), *args)
    return str(e.value)


def test_the_four_methods_refuse_k_zero_and_a_wrong_rank_in_their_own_words():
    import numpy as np
    assert _refusal("solve_tangent", np.zeros((0, 2, 4, 3))) == "dlod must have shape (K >= 1, 2, 4, 3) or lack the leading axis, got (0, 2, 4, 3)"
    assert _refusal("solve_tangent", np.zeros((4, 3))) == "dlod must have shape (K >= 1, 2, 4, 3) or lack the leading axis, got (4, 3)"
    assert _refusal("solve_tangent", np.zeros((2, 4, 5))) == "dlod must have shape (K >= 1, 2, 4, 3) or lack the leading axis, got (1, 2, 4, 5)"
    assert _refusal("solve_rhs", np.zeros((0, 2, 3))) == "rhs must have shape (K >= 1, 2, 3) or lack the leading axis, got (0, 2, 3)"
    assert _refusal("solve_rhs", np.zeros(3)) == "rhs must have shape (K >= 1, 2, 3) or lack the leading axis, got (3,)"
    assert _refusal("solve_rhs", np.zeros((2, 4))) == "rhs must have shape (K >= 1, 2, 3) or lack the leading axis, got (1, 2, 4)"
    dx = torch.zeros((2, 3), dtype=torch.float64)
    assert _refusal("solve_tangent_device", torch.zeros((0, 2, 4, 3), dtype=torch.float64), dx) == "solve_tangent_device: K == 0"
    assert _refusal("solve_tangent_device", torch.zeros((4, 3), dtype=torch.float64), dx) == \
        "solve_tangent_device: dlod must be a tensor of shape (K >= 1, batch, nVar + 1, cap) or (batch, nVar + 1, cap)"
    assert _refusal("solve_tangent_device", torch.zeros((2, 4, 3), dtype=torch.float64), torch.zeros((1, 2, 3), dtype=torch.float64)) == \
        "solve_tangent_device: dx must be a contiguous float64 tensor of shape (2, 3)"
    assert _refusal("solve_rhs_device", torch.zeros((0, 2, 3), dtype=torch.float64), dx) == "solve_rhs_device: K == 0"
    assert _refusal("solve_rhs_device", torch.zeros(3, dtype=torch.float64), dx) == "solve_rhs_device: rhs must be a tensor of shape (K >= 1, batch, cap) or (batch, cap)"
    assert _refusal("solve_rhs_device", torch.zeros((2, 2, 3), dtype=torch.float64), dx) == "solve_rhs_device: x must be a contiguous float64 tensor of shape (2, 2, 3)"
