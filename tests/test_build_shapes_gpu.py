"""GPU tests (MI355X): build_forest_kernel and build_extended_forest_kernel
against the CPU oracle, bit for bit, at the bag sizes, widths, seeds and
tree offsets the first parity tests leave out.

The cases and the reason each is there are in tests/test_build_shapes_ref.py,
which also checks, without a GPU, that each case reaches the code it names.
Here every case is built on the device and compared field by field with the
oracle's forest, the kernels' `depth` output included. Four cases go on
through the device-side scoring pack and, for standard forests, the scoring
walk: the raw build outputs past node_count are uninitialised memory, and
that step is what checks the packers mask them.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import IsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from isolation_forest_amd.utils.params import ResolvedParams  # noqa: E402
from tests.test_build_shapes_ref import (  # noqa: E402
    CHAIN_EXTENDED_IDS,
    CHAIN_STANDARD_IDS,
    EXT_FIELDS,
    EXTENDED_IDS,
    FIELDS,
    SHARDS,
    STANDARD_IDS,
    cpu_extended,
    cpu_standard,
    extended_case,
    field_bits,
    shard_of,
    standard_case,
    tree_slice,
)

_TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def assert_forest_identical(gpu_f, cpu_f, what=""):
    """Every field of a GPU-built forest equals the oracle's, floats as
    bits, and the kernel's depth output equals the depths of the oracle's
    tree on the live nodes."""
    extended = hasattr(cpu_f, "hyper_w")
    assert hasattr(gpu_f, "hyper_w") == extended
    for name in ["node_count", "feature", "right", "num_instances"]:
        np.testing.assert_array_equal(
            getattr(gpu_f, name), getattr(cpu_f, name),
            err_msg=f"{what} {name}")
    assert gpu_f.value.dtype == np.float32 == cpu_f.value.dtype
    np.testing.assert_array_equal(
        gpu_f.value.view(np.int32), cpu_f.value.view(np.int32),
        err_msg=f"{what} value")
    if extended:
        np.testing.assert_array_equal(gpu_f.hyper_idx, cpu_f.hyper_idx,
                                      err_msg=f"{what} hyper_idx")
        assert gpu_f.hyper_w.dtype == np.float32 == cpu_f.hyper_w.dtype
        np.testing.assert_array_equal(
            gpu_f.hyper_w.view(np.int32), cpu_f.hyper_w.view(np.int32),
            err_msg=f"{what} hyper_w")
        assert gpu_f.offset64.dtype == np.float64 == cpu_f.offset64.dtype
        np.testing.assert_array_equal(
            gpu_f.offset64.view(np.int64), cpu_f.offset64.view(np.int64),
            err_msg=f"{what} offset64")
    want = gpu_engine._node_depths(cpu_f.feature, cpu_f.right)
    cols = np.arange(cpu_f.feature.shape[1])[None, :]
    live = cols < cpu_f.node_count[:, None]
    assert gpu_f.depth_np.shape == want.shape, f"{what} depth"
    np.testing.assert_array_equal(gpu_f.depth_np[live], want[live],
                                  err_msg=f"{what} depth")


def _device_rows(X, dev, kind=None):
    Xt = torch.from_numpy(np.array(X)).to(dev)
    if kind is not None:
        # the case's rows are already 16-bit values: the narrowing is exact
        Xt = Xt.to(_TORCH_DTYPE[kind])
        np.testing.assert_array_equal(Xt.float().cpu().numpy(), X)
    return Xt


def _rp(a):
    return ResolvedParams(num_samples=a["n"], num_features=a["k"],
                          total_rows=a["N"], total_features=a["d"],
                          extension_level=a["extension_level"])


def _gpu_build(case, dev, kind=None):
    X, bag, fs, seed, a = case
    build = (gpu_engine.build_forest if a["extension_level"] is None
             else gpu_engine.build_extended_forest)
    return build(_device_rows(X, dev, kind), np.array(bag), np.array(fs),
                 seed, _rp(a), tree_id_offset=a["tree_id_offset"])


def _row_kind_of(cid):
    return cid.rsplit("-", 1)[1] if cid.startswith("S9") else None


class TestStandardBuildShapes:
    @pytest.mark.parametrize("cid", STANDARD_IDS)
    def test_identical_to_oracle(self, dev, cid):
        gpu_f = _gpu_build(standard_case(cid), dev, _row_kind_of(cid))
        assert_forest_identical(gpu_f, cpu_standard(cid), cid)

    def test_shards_concatenate_to_the_whole_forest(self, dev):
        """S7: trees [0, 3) and [3, 7) built with tree_id_offset 0 and 3."""
        whole = cpu_standard("S7")
        parts = [_gpu_build(shard_of(standard_case("S7"), lo, hi), dev)
                 for lo, hi in SHARDS]
        for name in FIELDS + ["depth_np"]:
            got = np.concatenate([getattr(p, name) for p in parts])
            want = (gpu_engine._node_depths(whole.feature, whole.right)
                    if name == "depth_np" else getattr(whole, name))
            if name == "depth_np":
                live = (np.arange(want.shape[1])[None, :]
                        < whole.node_count[:, None])
                got, want = got[live], want[live]
            np.testing.assert_array_equal(field_bits(got), field_bits(want),
                                          err_msg=f"S7 {name}")
        for (lo, hi), part in zip(SHARDS, parts):
            assert part.num_trees == hi - lo


class TestExtendedBuildShapes:
    @pytest.mark.parametrize("cid", EXTENDED_IDS)
    def test_identical_to_oracle(self, dev, cid):
        gpu_f = _gpu_build(extended_case(cid), dev)
        assert_forest_identical(gpu_f, cpu_extended(cid), cid)

    def test_shards_concatenate_to_the_whole_forest(self, dev):
        """E6: the S7 shard scheme on an extended forest."""
        whole = cpu_extended("E6-shards")
        parts = [_gpu_build(shard_of(extended_case("E6-shards"), lo, hi), dev)
                 for lo, hi in SHARDS]
        for name in EXT_FIELDS:
            got = np.concatenate([getattr(p, name) for p in parts])
            np.testing.assert_array_equal(
                field_bits(got), field_bits(getattr(whole, name)),
                err_msg=f"E6 {name}")
        for (lo, hi), part in zip(SHARDS, parts):
            sl = tree_slice(whole, lo, hi, ["feature", "right", "node_count"])
            want = gpu_engine._node_depths(sl["feature"], sl["right"])
            live = (np.arange(want.shape[1])[None, :]
                    < sl["node_count"][:, None])
            np.testing.assert_array_equal(part.depth_np[live], want[live],
                                          err_msg=f"E6 depth [{lo}, {hi})")


class TestDownstreamChain:
    """GPU-built forest -> device pack -> scoring walk, at an odd max_nodes
    with unwritten columns past node_count."""

    @pytest.mark.parametrize("cid", CHAIN_STANDARD_IDS)
    def test_standard_pack_and_path_sums(self, dev, cid):
        X, bag, fs, seed, a = standard_case(cid)
        d, T = a["d"], a["T"]
        forest = _gpu_build(standard_case(cid), dev)
        assert_forest_identical(forest, cpu_standard(cid), cid)
        raw = forest._device_raw
        assert raw["device"] == str(dev)
        for bf16 in (True, False):
            aos_dev, nc_dev, h_dev = gpu_engine._nodes_packed_v4_device(
                raw, forest.num_trees, d, bf16)
            aos_host, nc_host, h_host = gpu_engine._nodes_packed_v4(
                forest, d, bf16)
            np.testing.assert_array_equal(aos_dev.cpu().numpy(), aos_host)
            np.testing.assert_array_equal(nc_dev.cpu().numpy(), nc_host)
            assert h_dev == h_host

        Xs = np.random.RandomState(900 + d).normal(
            size=(257, d)).astype(np.float32)
        cpu_ps = cpu_engine.path_lengths(cpu_standard(cid), Xs)
        model = IsolationForest(numEstimators=T).fit(np.array(X[:600]))
        model.forest = forest  # shell for the pack cache
        model._gpu_forest_cache = {}
        gpu_ps = gpu_engine.score_forest(
            model, torch.from_numpy(Xs).to(dev), finalize=False)
        np.testing.assert_array_equal(
            gpu_ps.cpu().numpy().view(np.int32), cpu_ps.view(np.int32))

    @pytest.mark.parametrize("cid", CHAIN_EXTENDED_IDS)
    def test_extended_pack(self, dev, cid):
        forest = _gpu_build(extended_case(cid), dev)
        assert_forest_identical(forest, cpu_extended(cid), cid)
        raw = forest._device_raw
        assert raw["device"] == str(dev)
        aos_dev, vals_dev, hw_dev, h_dev = gpu_engine._eif_dense_packed_device(
            raw, 8)
        aos_host, vals_host, hw_host, h_host = gpu_engine._eif_dense_packed(
            forest, 8)
        np.testing.assert_array_equal(aos_dev.cpu().numpy(), aos_host)
        np.testing.assert_array_equal(vals_dev.cpu().numpy(), vals_host)
        np.testing.assert_array_equal(hw_dev.cpu().numpy(), hw_host)
        assert h_dev == h_host


class TestBuildCap:
    """Bags of more than 16384 rows: the bindings refuse them before any
    build launch, and the model builds such trees on the CPU instead."""

    N, D, T, SEED = 20000, 4, 2, 31

    def _args(self, level=None):
        X = np.random.RandomState(301).normal(
            size=(self.N, self.D)).astype(np.float32)
        bag = cpu_engine.sample_bags(self.N, self.T, 16385, seed=self.SEED,
                                     bootstrap=False)
        fs = cpu_engine.feature_subsets(self.D, self.D, self.T, self.SEED)
        rp = ResolvedParams(num_samples=16385, num_features=self.D,
                            total_rows=self.N, total_features=self.D,
                            extension_level=level)
        return X, bag, fs, rp

    def test_standard_binding_refuses_16385(self, dev):
        X, bag, fs, rp = self._args()
        with pytest.raises(RuntimeError, match="16384"):
            gpu_engine.build_forest(torch.from_numpy(X).to(dev), bag, fs,
                                    self.SEED, rp)

    def test_extended_binding_refuses_16385(self, dev):
        X, bag, fs, rp = self._args(level=1)
        with pytest.raises(RuntimeError, match="16384"):
            gpu_engine.build_extended_forest(
                torch.from_numpy(X).to(dev), bag, fs, self.SEED, rp)

    def test_fit_falls_back_to_cpu_build(self, dev):
        X, _, _, _ = self._args()
        gpu_m = IsolationForest(maxSamples=16385.0, numEstimators=2).fit(
            torch.from_numpy(X).to(dev))
        cpu_m = IsolationForest(maxSamples=16385.0, numEstimators=2).fit(
            torch.from_numpy(X))
        assert gpu_m.forest.num_samples == 16385 == cpu_m.forest.num_samples
        assert gpu_m.forest.feature.shape == (2, 2 * 16385 - 1)
        for name in FIELDS:
            np.testing.assert_array_equal(
                field_bits(getattr(gpu_m.forest, name)),
                field_bits(getattr(cpu_m.forest, name)), err_msg=name)
