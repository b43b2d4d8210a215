"""CPU: the pyramid's level sizes (keymorph_amd.io._pyramid.level_dims, what the three intensity drivers iterate over), and the
first branch of the similarity ops' argument checks: a CPU tensor raises KeymorphHipError before the library is touched."""
import pytest
import torch

from keymorph_amd import _lib, ops
from keymorph_amd.io._pyramid import level_dims


def test_level_dims_full_pyramid():
    assert level_dims((64, 64, 64), (4, 2, 1)) == [(16, 16, 16), (32, 32, 32), (64, 64, 64)]


def test_level_dims_drops_a_level_with_a_short_axis():
    assert level_dims((40, 64, 64), (4, 2, 1)) == [(20, 32, 32), (40, 64, 64)]      # 40 // 4 = 10 < 16


def test_level_dims_may_be_empty():
    assert level_dims((31, 64, 64), (2,)) == []                                       # 31 // 2 = 15 < 16


def test_level_dims_keeps_the_order_of_shrink():
    assert level_dims((64, 64, 64), (1, 4, 2)) == [(64, 64, 64), (16, 16, 16), (32, 32, 32)]


_VOL = torch.zeros(1, 1, 16, 16, 16)
_LATTICE = torch.zeros(1, 3, 5, 5, 5)
_CPU_CALLS = {
    "mutual_information": lambda: ops.mutual_information(_VOL, _VOL),
    "warp_mutual_information": lambda: ops.warp_mutual_information(_VOL, _VOL, torch.zeros(1, 3, 4)),
    "local_ncc": lambda: ops.local_ncc(_VOL, _VOL),
    "bspline_grid": lambda: ops.bspline_grid(_LATTICE, (16, 16, 16)),
    "bspline_bending": lambda: ops.bspline_bending(_LATTICE),
    "mi_ranges": lambda: ops.mi_ranges(_VOL, _VOL),
}


@pytest.mark.parametrize("name", list(_CPU_CALLS))
def test_cpu_tensor_raises_before_any_library_call(name, monkeypatch):
    def no_library():
        raise AssertionError(f"{name} reached the library with a CPU tensor")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(_lib.KeymorphHipError):
        _CPU_CALLS[name]()
