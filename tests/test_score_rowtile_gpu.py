"""GPU tests (MI355X) for dense rows past the v4 key tile:
score_forest_rowtile_kernel (ops/hip/rowtile_kernels.hip)
through gpu_engine.score_forest and the model. Every case builds a forest of
37 trees on 64-row bags on the CPU and compares path sums (once: finalized
scores) bitwise with cpu_engine.path_lengths on the same rows widened to f32.
The (R, G, PH, records in LDS) expected of score_rowtile_cfg are worked out by
hand from the rule in §3d."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import IsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine, load_extension  # noqa: E402
from tests.test_gpu_edges import Shell, _assert_bitwise  # noqa: E402
from tests.test_score_heap_ref import round_rows  # noqa: E402

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BITS = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}
TINY = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}
T = 37
# (kind, d) -> (R, G, PH, records in LDS) at maxSamples 64. The tile takes the
# largest R with R * 4 * SW <= 76800 and the records are read from L2 with
# four chains a lane. The first widths pick_score_cfg leaves without a key
# tile are 16-bit d = 300 and f32 d = 150: up to 299 / 149 a 256-row tile
# still fits once the records go to L2, and that v4 walk scored 81 M rows/s
# against 52 M here (profiles/score_rowtile.md), so it keeps those widths and
# G = 2 is reached with IFA_SCORE_ROWTILE=1 only.
CFG = {("bf16", 300): (64, 4, 16, False), ("f32", 150): (64, 4, 16, False),
       ("f16", 600): (32, 8, 32, False), ("bf16", 1200): (16, 16, 64, False),
       ("f32", 2047): (8, 32, 128, False), ("bf16", 4094): (8, 32, 128, False),
       ("f32", 4094): (4, 64, 256, False)}
FORCED = {("bf16", 296): (128, 2, 8, False), ("f32", 148): (128, 2, 8, False),
          ("bf16", 5): (256, 1, 4, False)}
# IFA_ROWTILE_RECORDS=lds: 127 records a tree are 1016 B; beside the 65568 B
# tile of f32 d = 2047 fit 82 trees, 2 for each of the 32 lanes
STAGED = {("f16", 600): (32, 8, 32, True), ("f32", 2047): (8, 32, 64, True)}
_MEMO = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _round(X, kind):
    return np.float32(X) if kind == "f32" else round_rows(X, kind)


def _rows(N, d, kind, seed=0):
    """Gaussian rows, exact in the row kind."""
    key = ("rows", N, d, kind, seed)
    if key not in _MEMO:
        _MEMO[key] = _round(np.random.RandomState(
            1000 * seed + d).standard_normal((N, d)), kind)
    return _MEMO[key].copy()


def _forest(d, kind, n=64, feats=None):
    key = ("forest", d, kind, n, feats)
    if key not in _MEMO:
        X = _rows(n + 300, d, kind, seed=7)
        bag = cpu_engine.sample_bags(n + 300, T, n, seed=17, bootstrap=False)
        fs = (cpu_engine.feature_subsets(d, d, T, seed=17) if feats is None
              else np.tile(np.int32(feats), (T, 1)))
        _MEMO[key] = cpu_engine.build_forest(X, bag, fs, 17, n, fs.shape[1], d)
    return _MEMO[key]


def _shape(forest, d, kind):
    n = forest.num_samples
    return kind, d, forest.feature.shape[1], max(int(np.ceil(np.log2(n))), 1)


def _to_dev(X, kind, dev):
    return torch.from_numpy(X).to(KINDS[kind]).to(dev)  # exact: X is rounded


def _check(dev, forest, X, kind, what, view=None, route="rowtile", cfg=CFG):
    """Assert the route and the configuration, score, compare bitwise."""
    d, ext = X.shape[1], load_extension()
    assert ext.score_route(*_shape(forest, d, kind), "packed") == route, what
    assert tuple(ext.score_rowtile_cfg(*_shape(forest, d, kind))) == \
        cfg[kind, d], what
    Xt = _to_dev(X, kind, dev) if view is None else view
    got = gpu_engine.score_forest(Shell(forest), Xt, finalize=False)
    with np.errstate(all="ignore"):
        want = cpu_engine.path_lengths(forest, X)
    _assert_bitwise(got.cpu().numpy(), want, what)
    return got


@pytest.mark.parametrize("kind, d, table", [
    (k, d, t) for t in ("CFG", "FORCED", "STAGED") for k, d in globals()[t]])
def test_lane_widths(dev, monkeypatch, kind, d, table):
    forest, cfg = _forest(d, kind), globals()[table]
    if table == "FORCED":  # over the heap and v4 routes
        assert load_extension().score_route(
            *_shape(forest, d, kind), "packed") in ("heap", "v4_global_nodes")
        monkeypatch.setenv("IFA_SCORE_ROWTILE", "1")
    if table == "STAGED":
        monkeypatch.setenv("IFA_ROWTILE_RECORDS", "lds")
    _check(dev, forest, _rows(2 * cfg[kind, d][0] + 1, d, kind), kind,
           f"{kind} d={d} {table}", cfg=cfg)


def _step(v, kind, up):
    """The neighbour of a non-zero finite v in the row's type."""
    t = torch.tensor([v], dtype=KINDS[kind])
    t.view(BITS[kind]).add_(1 if (v > 0) == up else -1)
    return float(t.float())


@pytest.mark.parametrize("kind, d", [("bf16", 300), ("f32", 150)])
def test_cells(dev, kind, d):
    """Thresholds of the row's own walk and their neighbours, zeros,
    denormals, the largest finite values and non-finite values, in cells that
    every walk reads: each tree splits its root on column d - 1, 0 or 7."""
    cols = (d - 1, 0, 7)
    forest = _forest(d, kind, feats=cols)
    roots = forest.feature[:, 0]
    assert set(roots.tolist()) == set(cols)  # every root is internal
    thr = gpu_engine._split_thresholds32(forest)[:, 0]
    fi = torch.finfo(KINDS[kind])
    special = np.float32([0.0, -0.0, TINY[kind], -TINY[kind],
                          fi.tiny - TINY[kind], fi.max, -fi.max, np.nan,
                          np.inf, -np.inf])
    X = _rows(3 * T + len(special), d, kind, seed=3)
    for t in range(T):  # rows 3t .. 3t + 2 meet the root of tree t
        v = float(_round(thr[t:t + 1], kind)[0])
        X[3 * t:3 * t + 3, roots[t]] = [v, _step(v, kind, False),
                                       _step(v, kind, True)]
    for i in range(len(special)):  # each value in each of the columns once
        X[3 * T + i, cols] = np.roll(special, i)[:3]
    with np.errstate(all="ignore"):  # the step across a threshold moves a walk
        low, high = X.copy(), X.copy()
        low[:3 * T, cols], high[:3 * T, cols] = -np.inf, np.inf
        assert (cpu_engine.path_lengths(forest, low)[:3 * T]
                != cpu_engine.path_lengths(forest, high)[:3 * T]).any()
    _check(dev, forest, X, kind, f"cells {kind}")


@pytest.mark.parametrize("layout", ["packed", "pitched", "odd pitch, base off",
                                    "feature-major"])
def test_layouts(dev, layout):
    d, kind = 600, "f16"
    forest, X = _forest(d, kind), _rows(70, d, kind, seed=5)
    N, packed = len(X), _to_dev(X, kind, dev)
    if layout == "packed":
        view = packed
    elif layout == "pitched":
        view = torch.zeros((N, d + 8), dtype=packed.dtype, device=dev)[:, :d]
        assert view.data_ptr() % 16 == 0
    elif layout == "odd pitch, base off":  # odd rows start off a word
        flat = torch.zeros(N * (d + 1) + 1, dtype=packed.dtype, device=dev)
        view = flat[1:].view(N, d + 1)[:, :d]
        assert view.data_ptr() % 4 == 2 and view.stride(0) % 2 == 1
    else:
        view = torch.zeros((d, N + 5), dtype=packed.dtype, device=dev)[:, :N].T
        assert view.stride() == (1, N + 5)
    view.copy_(packed)
    got = _check(dev, forest, X, kind, layout, view=view)
    want = gpu_engine.score_forest(Shell(forest), view.contiguous(),
                                   finalize=False)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("kind, d", [("bf16", 300), ("f32", 2047)])
@pytest.mark.parametrize("N", ["1", "R-1", "R+1", "3R+5"])
def test_row_counts_in_one_block(dev, monkeypatch, N, kind, d):
    monkeypatch.setenv("IFA_ROWTILE_MAX_BLOCKS", "1")
    R = CFG[kind, d][0]
    N = {"1": 1, "R-1": R - 1, "R+1": R + 1, "3R+5": 3 * R + 5}[N]
    _check(dev, _forest(d, kind), _rows(N, d, kind, seed=N), kind,
           f"N={N} d={d}")


def test_switched_off(dev, monkeypatch):
    monkeypatch.setenv("IFA_SCORE_ROWTILE", "0")
    _check(dev, _forest(600, "f16"), _rows(300, 600, "f16"), "f16",
           "switched off", route="v4_global_rows")


def test_finalized_scores(dev):
    d, kind = 1200, "bf16"
    forest, X = _forest(d, kind), _rows(40, d, kind)
    got = gpu_engine.score_forest(Shell(forest), _to_dev(X, kind, dev))
    want = cpu_engine.scores_from_path_sums(
        cpu_engine.path_lengths(forest, X), forest.num_trees,
        forest.num_samples)
    _assert_bitwise(got.cpu().numpy(), want, "finalized")


def test_fit_on_the_model(dev):
    X = torch.from_numpy(_rows(3000, 600, "bf16", seed=9)).to(torch.bfloat16)
    make = lambda: IsolationForest(  # noqa: E731
        numEstimators=T, maxSamples=64, contamination=0.05)
    gpu_m, cpu_m = make().fit(X.to(dev)), make().fit(X)
    for name in ("feature", "value", "right", "num_instances", "node_count"):
        assert np.array_equal(getattr(gpu_m.forest, name),
                              getattr(cpu_m.forest, name)), name
    assert (np.float64(gpu_m.outlier_score_threshold).tobytes()
            == np.float64(cpu_m.outlier_score_threshold).tobytes())
    assert torch.equal(gpu_m.score(X.to(dev)).cpu().view(torch.int32),
                       torch.as_tensor(cpu_m.score(X)).view(torch.int32))
