"""GPU tests (MI355X) for sparse CSR input: score_forest_csr_kernel and
bag_gather_csr_kernel (ops/hip/csr_kernels.hip) through gpu_engine and the
models. Every scoring case first asserts the (R, G, PH, records in LDS) that
score_csr_cfg reports, worked out by hand from the rule in DESIGN.md §3c,
then compares the path sums bitwise with cpu_engine.path_lengths on the dense
matrix, for a forest the CPU built on dense rows."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import IsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine, load_extension  # noqa: E402
from tests.test_gpu_edges import Shell, _assert_bitwise  # noqa: E402
from tests.test_score_heap_ref import round_rows, split_rows  # noqa: E402

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TINY = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}
# (R, G, PH, records in LDS) for maxSamples 64 (127 records a tree)
CFG = {(1, 2): (256, 1, 4, True), (1, 4): (256, 1, 4, True),
       (5, 2): (256, 1, 4, True), (5, 4): (256, 1, 4, True),
       (300, 2): (64, 4, 16, True), (300, 4): (32, 8, 32, True),
       (1000, 2): (32, 8, 32, True), (1000, 4): (16, 16, 64, True),
       (4094, 2): (8, 32, 64, True), (4094, 4): (4, 64, 64, True)}
_MEMO = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _rows(N, d, kind, seed=0):
    """About 90 % zeros, both signs elsewhere, exact in the row kind."""
    key = ("rows", N, d, kind, seed)
    if key not in _MEMO:
        rs = np.random.RandomState(1000 * seed + d)
        X = rs.standard_normal((N, d)).astype(np.float32)
        X[rs.random_sample((N, d)) < 0.9] = 0.0
        _MEMO[key] = X if kind == "f32" else round_rows(X, kind)
    return _MEMO[key].copy()


def _forest(d, kind, n=64, T=9, feats=None, constant=False):
    key = ("forest", d, kind, n, T, feats, constant)
    if key not in _MEMO:
        rows = n + 300
        X = (np.full((rows, d), 1.5, dtype=np.float32) if constant
             else _rows(rows, d, kind, seed=7))
        bag = cpu_engine.sample_bags(rows, T, n, seed=17, bootstrap=False)
        fs = (cpu_engine.feature_subsets(d, d, T, seed=17) if feats is None
              else np.tile(np.int32(feats), (T, 1)))
        _MEMO[key] = cpu_engine.build_forest(X, bag, fs, 17, n, fs.shape[1], d)
    return _MEMO[key]


def _csr(X, kind, dev, stored=None, idtype=torch.int32):
    """X as CSR: every non-zero cell, plus the cells `stored` marks."""
    mask = X != 0  # NaN included
    if stored is not None:
        mask = mask | stored
    crow = np.concatenate([[0], np.cumsum(mask.sum(1))])
    return torch.sparse_csr_tensor(
        torch.from_numpy(crow).to(idtype).to(dev),
        torch.from_numpy(np.nonzero(mask)[1]).to(idtype).to(dev),
        torch.from_numpy(X[mask]).to(KINDS[kind]).to(dev), size=X.shape)


def _check(dev, forest, X, kind, cfg, what, **csr):
    d, n = X.shape[1], forest.num_samples
    got_cfg = load_extension().score_csr_cfg(
        kind, d, forest.feature.shape[1], max(int(np.ceil(np.log2(n))), 1))
    assert tuple(got_cfg) == cfg, what
    got = gpu_engine.score_forest_csr(Shell(forest), _csr(X, kind, dev, **csr),
                                      finalize=False)
    with np.errstate(all="ignore"):
        want = cpu_engine.path_lengths(forest, X)
    _assert_bitwise(got.cpu().numpy(), want, what)


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("d", [1, 5, 300, 1000, 4094])
def test_group_widths(dev, d, kind):
    cfg = CFG[d, KINDS[kind].itemsize]
    wide = d == 4094
    forest = _forest(d, kind, feats=(4093, 0, 2047) if wide else None)
    X = _rows(cfg[0] + 3, d, kind)
    if wide:  # the last column is split on and stored
        X[::2, 4093] = 1.0
        assert (forest.feature == 4093).any()
    _check(dev, forest, X, kind, cfg, f"d={d} {kind}")


@pytest.mark.parametrize("d, kind", [(5, "f32"), (300, "bf16")])
@pytest.mark.parametrize("N", ["1", "R-1", "R+1", "2R+1 in one block"])
def test_row_counts(dev, monkeypatch, N, d, kind):
    cfg = CFG[d, KINDS[kind].itemsize]
    R = cfg[0]
    if N.endswith("one block"):
        monkeypatch.setenv("IFA_CSR_MAX_BLOCKS", "1")
    N = {"1": 1, "R-1": R - 1, "R+1": R + 1}.get(N, 2 * R + 1)
    _check(dev, _forest(d, kind), _rows(N, d, kind, seed=N), kind, cfg,
           f"N={N} d={d}")


def test_row_shapes(dev):
    d, kind = 300, "bf16"  # G = 4
    X = _rows(70, d, kind)
    X[[0, 5, 69]] = 0.0                      # empty rows, the last included
    X[2] = np.abs(_rows(1, d, kind, seed=3)[0]) + 1.0  # full: nnz = d
    X[3] = 0.0
    X[3, 10:50] = -2.0                       # 40 entries > 4 G
    X[4] = 0.0
    X[4, 0] = 3.0                            # column 0 only
    X[6] = 0.0
    X[6, d - 1] = -3.0                       # column d - 1 only
    _check(dev, _forest(d, kind), X, kind, CFG[d, 2], "row shapes")
    _check(dev, _forest(d, kind), np.zeros((70, d), dtype=np.float32), kind,
           CFG[d, 2], "nnz = 0")


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_values(dev, kind):
    d = 300
    forest = _forest(d, kind)
    X = _rows(100, d, kind)
    X[:40] = split_rows(forest, 40, d, kind)  # equality goes right
    special = np.float32([0.0, -0.0, np.nan, np.inf, -np.inf, TINY[kind],
                          -TINY[kind]])
    for i in range(7):  # each special value in every column of 0 .. 6 once
        X[40 + i, :7] = np.roll(special, i)
    stored = np.zeros(X.shape, dtype=bool)
    stored[40:47, :7] = True  # 0.0 and -0.0 are stored entries
    _check(dev, forest, X, kind, CFG[d, KINDS[kind].itemsize],
           f"values {kind}", stored=stored)


@pytest.mark.parametrize("d, kind", [(5, "f32"), (300, "bf16")])
def test_int64_indices(dev, d, kind):
    cfg = CFG[d, KINDS[kind].itemsize]
    _check(dev, _forest(d, kind), _rows(cfg[0] + 9, d, kind, seed=4), kind,
           cfg, "int64 indices", idtype=torch.int64)


@pytest.mark.parametrize("T", [1, 16, 17])  # 1, PH, PH + 1
def test_tree_counts(dev, T):
    _check(dev, _forest(300, "bf16", T=T), _rows(67, 300, "bf16"), "bf16",
           CFG[300, 2], f"T={T}")


def test_constant_training_data(dev):
    forest = _forest(300, "f16", constant=True)
    assert (forest.node_count == 1).all()  # every root is a leaf
    _check(dev, forest, _rows(67, 300, "f16"), "f16", CFG[300, 2], "constant")


def test_records_outside_lds(dev):
    d, kind, ext = 1000, "f16", load_extension()
    n = next(n for n in range(2, 16385)
             if not ext.score_csr_cfg(kind, d, 2 * n - 1, 10)[3])
    # G = 8 lanes need 8 trees of 8 (2n - 1) bytes in the 85376 B beside the
    # 64128 B tile and the 4096 B of slots: n <= 667
    assert n == 668
    _check(dev, _forest(d, kind, n=n, T=17), _rows(67, d, kind), kind,
           (64, 4, 16, False), "records from L2")  # two phases


def test_finalized_scores(dev):
    d, kind = 300, "bf16"
    forest, X = _forest(d, kind), _rows(67, d, kind)
    got = gpu_engine.score_forest_csr(Shell(forest), _csr(X, kind, dev))
    want = cpu_engine.scores_from_path_sums(
        cpu_engine.path_lengths(forest, X), forest.num_trees,
        forest.num_samples)
    _assert_bitwise(got.cpu().numpy(), want, "finalized")


def test_fit_equals_dense_fit(dev):
    Xd = torch.from_numpy(_rows(3000, 40, "f32")).to(dev)
    est = IsolationForest(numEstimators=9, maxSamples=64, contamination=0.05)
    ms, md = est.fit(Xd.to_sparse_csr()), est.fit(Xd)
    for name in ("feature", "value", "right", "num_instances", "node_count",
                 "value64"):
        assert np.array_equal(getattr(ms.forest, name),
                              getattr(md.forest, name)), name
    assert (np.float64(ms.outlier_score_threshold).tobytes()
            == np.float64(md.outlier_score_threshold).tobytes())


@pytest.mark.parametrize("kind, idtype", [("f32", torch.int64),
                                          ("bf16", torch.int32),
                                          ("f16", torch.int64)])
def test_bag_gather(dev, kind, idtype):
    X = _rows(50, 37, kind)
    X[7] = 0.0  # an empty row, drawn twice below
    X[3, 5] = -0.0
    stored = np.zeros(X.shape, dtype=bool)
    stored[3, 5] = True
    Xs = _csr(X, kind, dev, stored=stored, idtype=idtype)
    bag = torch.tensor([[7, 3, 3, 49, 0, 3], [1, 7, 48, 2, 2, 48]], device=dev)
    got = load_extension().bag_gather_csr(
        Xs.crow_indices(), Xs.col_indices(), Xs.values(), 37, bag)
    want = load_extension().bag_gather(
        torch.from_numpy(X).to(KINDS[kind]).to(dev), bag)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
