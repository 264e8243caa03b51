"""GPU tests (MI355X): build_forest_large_kernel and
build_extended_forest_large_kernel (bags of more than 16384 rows) against
the CPU oracle, bit for bit.

The cases and the reason each is there are in tests/test_build_large_ref.py.
Here every case is built on the device through gpu_engine.build_forest_large
/ build_extended_forest_large and compared field by field with the oracle's
forest, the kernels' `depth` output included; then the same bag is built
from 16-bit, pitched and feature-major rows, in one-tree chunks, and through
the two estimators' fit().
"""

import logging

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
from isolation_forest_amd.utils.params import ResolvedParams  # noqa: E402
from tests.test_build_large_ref import (  # noqa: E402
    EXTENDED_LARGE_IDS,
    STANDARD_LARGE_IDS,
    cpu_large,
    is_extended,
    large_case,
)
from tests.test_build_shapes_gpu import assert_forest_identical  # noqa: E402
from tests.test_build_shapes_ref import (  # noqa: E402
    EXT_FIELDS,
    FIELDS,
    build_extended,
    build_standard,
    field_bits,
    round_rows16,
)

_TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _rp(a):
    return ResolvedParams(num_samples=a["n"], num_features=a["k"],
                          total_rows=a["N"], total_features=a["d"],
                          extension_level=a["extension_level"])


def _build_large(case, Xt, **kw):
    """The forest with the kernel's depths attached the way the small
    builders attach them, which is where assert_forest_identical looks."""
    X, bag, fs, seed, a = case
    build = (gpu_engine.build_forest_large if a["extension_level"] is None
             else gpu_engine.build_extended_forest_large)
    forest, depth = build(Xt, np.array(bag), np.array(fs), seed, _rp(a),
                          tree_id_offset=a["tree_id_offset"],
                          return_depth=True, **kw)
    # the large builders leave nothing on the forest for the device packers
    assert not hasattr(forest, "_device_raw")
    assert getattr(forest, "depth_np", None) is None
    forest.depth_np = depth
    return forest


def _assert_same_build(got, want, what):
    fields = EXT_FIELDS if hasattr(want, "hyper_w") else FIELDS
    for name in fields + ["depth_np"]:
        np.testing.assert_array_equal(
            field_bits(getattr(got, name)), field_bits(getattr(want, name)),
            err_msg=f"{what} {name}")


class TestLargeBuildIdenticalToOracle:
    @pytest.mark.parametrize("cid", STANDARD_LARGE_IDS + EXTENDED_LARGE_IDS)
    def test_identical_to_oracle(self, dev, cid):
        case = large_case(cid)
        forest = _build_large(case, torch.from_numpy(np.array(case[0])).to(dev))
        assert hasattr(forest, "hyper_w") == is_extended(cid)
        assert_forest_identical(forest, cpu_large(cid), cid)

    def test_old_bindings_still_refuse_16385(self, dev):
        X, bag, fs, seed, a = large_case("L1")
        with pytest.raises(RuntimeError, match="16384"):
            gpu_engine.build_forest(torch.from_numpy(np.array(X)).to(dev),
                                    np.array(bag), np.array(fs), seed, _rp(a))


class TestLargeBuildRowFormats:
    """L1 from 16-bit rows and from strided views: rows are read in place,
    widened exactly, and the forest does not depend on where they lie."""

    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("cid", ["L1", "X1-full"])
    def test_16_bit_rows(self, dev, cid, kind):
        X, bag, fs, seed, a = large_case(cid)
        X16 = round_rows16(X, kind)  # values exact in 16 bits, as f32
        assert (X16 != X).any()
        case16 = (X16, bag, fs, seed, a)
        want = (build_extended if is_extended(cid) else build_standard)(case16)
        X16_t = torch.from_numpy(X16).to(dev)
        narrow = X16_t.to(_TORCH_DTYPE[kind])
        np.testing.assert_array_equal(narrow.float().cpu().numpy(), X16)
        got = _build_large(case16, narrow)
        assert_forest_identical(got, want, f"{cid} {kind}")
        # and bitwise the packed f32 build of the same values
        _assert_same_build(got, _build_large(case16, X16_t), f"{cid} {kind}")

    @pytest.mark.parametrize("cid", ["L1", "X1-nnz2k3"])
    def test_pitched_and_feature_major_views(self, dev, cid):
        case = large_case(cid)
        X = np.array(case[0])
        N, d = X.shape
        packed = _build_large(case, torch.from_numpy(X).to(dev))
        assert_forest_identical(packed, cpu_large(cid), cid)

        table = torch.full((N, d + 3), float("nan"), device=dev)
        table[:, 1:1 + d] = torch.from_numpy(X).to(dev)
        pitched = table[:, 1:1 + d]
        assert pitched.stride() == (d + 3, 1) and not pitched.is_contiguous()
        _assert_same_build(_build_large(case, pitched), packed,
                           f"{cid} pitched")

        fm = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev).T
        assert fm.shape == (N, d) and fm.stride() == (1, N)
        _assert_same_build(_build_large(case, fm), packed,
                           f"{cid} feature-major")


class TestLargeBuildChunks:
    @pytest.mark.parametrize("level", [None, 1])
    def test_one_tree_chunks_equal_a_single_launch(self, dev, level):
        X = np.array(large_case("L1")[0])
        N, d = X.shape
        T, n, seed = 3, 16385, 47
        bag = cpu_engine.sample_bags(N, T, n, seed=seed, bootstrap=False)
        fs = cpu_engine.feature_subsets(d, d, T, seed)
        a = {"n": n, "k": d, "N": N, "d": d, "extension_level": level,
             "tree_id_offset": 0}
        case = (X, bag, fs, seed, a)
        Xt = torch.from_numpy(X).to(dev)
        whole = _build_large(case, Xt, chunk_trees=T)
        parts = _build_large(case, Xt, chunk_trees=1)
        assert whole.num_trees == T == parts.num_trees
        _assert_same_build(parts, whole, f"chunks level={level}")
        # the trees differ, so a chunk built with the wrong offset would show
        assert len({whole.value[t].tobytes() for t in range(T)}) == T
        with pytest.raises(ValueError):
            _build_large(case, Xt, chunk_trees=-1)


class TestLargeBuildThroughFit:
    """fit() on a CUDA tensor with maxSamples > 16384 builds on the device
    and gives the forest and the scores of the same fit on the CPU tensor."""

    @pytest.mark.parametrize("est,n", [(IsolationForest, 20000.0),
                                       (ExtendedIsolationForest, 17000.0)])
    def test_fit_builds_on_the_device(self, dev, caplog, est, n):
        X = np.array(large_case("L2")[0])[:, :6].copy()
        X += np.random.RandomState(408).normal(size=X.shape).astype(np.float32)
        Xc = torch.from_numpy(X)
        with caplog.at_level(logging.WARNING):
            gpu_m = est(maxSamples=n, numEstimators=2).fit(Xc.to(dev))
        assert "building trees on CPU" not in caplog.text
        cpu_m = est(maxSamples=n, numEstimators=2).fit(Xc)
        assert gpu_m.forest.num_samples == int(n) == cpu_m.forest.num_samples
        fields = EXT_FIELDS if est is ExtendedIsolationForest else FIELDS
        for name in fields:
            np.testing.assert_array_equal(
                field_bits(getattr(gpu_m.forest, name)),
                field_bits(getattr(cpu_m.forest, name)), err_msg=name)
        assert not hasattr(gpu_m.forest, "_device_raw")
        Xs = Xc[:3000]
        got = gpu_m.score(Xs.to(dev)).cpu().numpy()
        want = cpu_m.score(Xs).numpy()
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
