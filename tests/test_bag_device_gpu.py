"""GPU tests (MI355X): gpu_engine.sample_bags_device (ops/hip/bag_kernels.hip)
against cpu_engine.sample_bags with the same arguments, bit for bit, on every
route: the LDS hash table, the global-memory table, the dense regime's sorted
keys and bootstrap; then through fit() of both estimators with the host
sampler made to raise.

Cases are (N, T, n, seed, tree_id_offset). The collision-heavy ones sit near
N = 2n, where the oracle runs 4 to 15 redraw rounds and settled slots are
displaced by smaller ones.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import (  # noqa: E402
    ExtendedIsolationForest,
    IsolationForest,
)
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests.test_build_shapes_ref import (  # noqa: E402
    EXT_FIELDS,
    FIELDS,
    same_forest,
)

L = gpu_engine.BAG_LDS_MAX_SAMPLES

SPARSE = [
    # LDS route, collision-heavy
    (512, 8, 256, 1, 0),
    (600, 8, 256, 2, 5),
    (100, 4, 50, 3, 0),  # n not a power of two
    (130, 4, 64, 9, 0),
    (129, 3, 64, 9, 0),  # N = 2n + 1
    (128, 3, 64, 9, 0),  # N = 2n, still the sparse regime
    # no collision at all: the flagship's usual case
    (20_000_000, 8, 256, 8, 0),
    # route boundary
    (2 * L + 1, 2, L, 5, 0),
    (2 * (L + 1) + 1, 2, L + 1, 5, 0),
    # global route
    (20000, 2, 8193, 4, 0),
    (32770, 2, 16385, 6, 1000),
    (140000, 2, 70000, 7, 0),
]
DENSE = [(127, 3, 64, 1, 0), (256, 20, 256, 1, 0), (32000, 2, 16385, 2, 3)]
BOOTSTRAP = [(1000, 4, 256, 1, 0), (50, 4, 200, 4, 2)]  # second: n > N


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def assert_same_bags(got, N, T, n, seed, bootstrap, off, row_offset=0):
    want = cpu_engine.sample_bags(N, T, n, seed, bootstrap, tree_id_offset=off,
                                  row_offset=row_offset)
    assert got.is_cuda and got.dtype == torch.int64
    got = got.cpu().numpy()
    assert got.shape == want.shape == (T, n) and want.dtype == np.int64
    assert np.array_equal(got, want)


@pytest.mark.parametrize("N,T,n,seed,off", SPARSE + DENSE)
def test_without_replacement(dev, N, T, n, seed, off):
    got = gpu_engine.sample_bags_device(N, T, n, seed, False,
                                        tree_id_offset=off, device=dev)
    assert_same_bags(got, N, T, n, seed, False, off)


@pytest.mark.parametrize("N,T,n,seed,off", BOOTSTRAP)
def test_bootstrap(dev, N, T, n, seed, off):
    got = gpu_engine.sample_bags_device(N, T, n, seed, True,
                                        tree_id_offset=off, device=dev)
    assert_same_bags(got, N, T, n, seed, True, off)


@pytest.mark.parametrize("N,n,bootstrap", [
    (600, 256, False), (20000, 8193, False), (127, 64, False),
    (1000, 256, True)])
def test_row_offset(dev, N, n, bootstrap):
    got = gpu_engine.sample_bags_device(N, 2, n, 3, bootstrap,
                                        tree_id_offset=1, row_offset=10 ** 10,
                                        device=dev)
    assert_same_bags(got, N, 2, n, 3, bootstrap, 1, row_offset=10 ** 10)


def test_lds_slot_state_in_the_output_row(dev):
    """A 64-thread block over 1000 slots is past 8 slots per thread: the
    kernel keeps its slot state in the output row (returns 0)."""
    from isolation_forest_amd.ops import load_extension

    out = torch.empty((3, 1000), dtype=torch.int64, device=dev)
    assert load_extension().bag_sample_lds(out, 2001, 4, 7, 0, 64) == 0
    assert_same_bags(out, 2001, 3, 1000, 4, False, 7)


def test_more_samples_than_rows_raises(dev):
    with pytest.raises(ValueError):
        gpu_engine.sample_bags_device(100, 2, 101, 1, False, device=dev)


@pytest.mark.parametrize("n", [256, 16385])
@pytest.mark.parametrize("cls,fields", [(IsolationForest, FIELDS),
                                        (ExtendedIsolationForest, EXT_FIELDS)])
def test_fit_draws_on_the_device(dev, monkeypatch, cls, fields, n):
    X = torch.from_numpy(np.random.RandomState(n).normal(
        size=(40000, 4)).astype(np.float32)).to(dev)
    est = cls(numEstimators=2, maxSamples=float(n), randomSeed=11)
    monkeypatch.setenv("IFA_BAG_DEVICE", "0")
    host = est.fit(X).forest

    def no_host_sampler(*a, **kw):
        raise AssertionError("fit() drew its bags on the host")

    monkeypatch.delenv("IFA_BAG_DEVICE")
    monkeypatch.setattr(cpu_engine, "sample_bags", no_host_sampler)
    assert same_forest(est.fit(X).forest, host, fields)
