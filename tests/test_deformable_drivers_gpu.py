"""GPU: what io.register_bspline and io.register_svf have in common because they are one loop (io/_deformable.py: fit_lattice and
metric_table), asserted once over both drivers and all three metrics -- a batch equals its single runs, a level does not wait for
the GPU, metric="mi" is the default, and the refusals.  What each driver and each metric recovers is in its own file
(tests/test_bspline_gpu.py, test_svf_gpu.py, test_lncc_gpu.py, test_mind_gpu.py).

Everything is at the restatements' own 32^3 pairs, each validated in its CPU file, from the identity matrix."""
import pytest
import torch

from tests import bspline_ref as B
from tests import lncc_ref
from tests import mind_ref
from tests import svf_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DRIVERS = ("register_bspline", "register_svf")
METRICS = ("mi", "lncc", "mind")


def driver_of(name):
    from keymorph_amd import io
    return getattr(io, name)


def pair(driver, metric):
    """Pair 0, (fixed, moving) on the GPU: the metric's own validated pair."""
    if metric == "mi":
        fixed, moving = svf_ref.recovery_pair() if driver == "register_svf" else B.recovery_pair()
    else:
        fixed, moving = lncc_ref.biased_pair() if metric == "lncc" else mind_ref.inverted_pair()
    return fixed.to(DEV), moving.to(DEV)


def identity_mat(n=1):
    from keymorph_amd.io import voxel_to_mat
    return voxel_to_mat(torch.eye(3, device=DEV)[None].expand(n, 3, 3), torch.zeros(n, 3, device=DEV), (B.SIZE,) * 3)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("driver", DRIVERS)
def test_batch_equals_single_runs(driver, metric):
    """The default schedule on two pairs at once against the two pairs alone, bit for bit."""
    register = driver_of(driver)
    f, m = pair(driver, metric)
    f2, m2 = (t.to(DEV) for t in B.recovery_pair(seed=4))
    both = register(torch.cat([f, f2]), torch.cat([m, m2]), mat=identity_mat(2), metric=metric)
    assert torch.equal(both[0], register(f, m, mat=identity_mat(), metric=metric)[0])
    assert torch.equal(both[1], register(f2, m2, mat=identity_mat(), metric=metric)[0])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("driver", DRIVERS)
def test_does_not_wait_for_the_gpu(driver, metric):
    """One full-resolution level under torch's synchronisation check, after a first call that allocates."""
    register = driver_of(driver)
    f, m = pair(driver, metric)
    mat = identity_mat()
    first = register(f, m, mat=mat, shrink=(1,), iters=3, metric=metric)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = register(f, m, mat=mat, shrink=(1,), iters=3, metric=metric)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, again) and torch.isfinite(first).all()


@pytest.mark.parametrize("driver", DRIVERS)
def test_default_metric_and_refusals(driver):
    register = driver_of(driver)
    f, m = pair(driver, "mi")
    mat = identity_mat()
    assert torch.equal(register(f, m, mat=mat, iters=5, metric="mi"), register(f, m, mat=mat, iters=5))
    refused = [dict(mat=mat, metric="ncc"), dict(mat=mat, metric="mind", mind_radius=4), dict(mat=identity_mat(2))]
    if driver == "register_svf":
        refused += [dict(mat=mat, steps=13), dict(mat=mat, steps=True)]
    for kwargs in refused:
        with pytest.raises(ValueError):
            register(f, m, **kwargs)
    with pytest.raises(ValueError):
        register(f, m[..., :-1], mat=mat)
