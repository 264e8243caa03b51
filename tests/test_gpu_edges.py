"""GPU edge tests (MI355X): non-finite / denormal rows, the second
grid-stride iteration, and every shipped route switch.

The parity tests in tests/test_gpu.py and tools/fuzz_parity.py use Gaussian
data. This file feeds the same kernels the float edge cases (+-0,
denormals, +-FLT_MIN, +-inf, NaN, +-3e38), scores enough rows to reach the
second iteration of every scoring kernel's grid-stride loop, and pins each
test to a NAMED kernel: router calls are observed through a recording proxy
of the extension, direct binding calls recompute the binding's own
instantiation predicate. Oracle: the strict-order CPU engine.

Dense contract (reassociated dots, PARITY.md): of 3001 rows at most 3 may
differ from the oracle path sum by more than 1e-3, each one explained as a
knife edge by tools/fuzz_parity.py::_knife_edge_explained; rows holding a
non-finite cell must match bitwise. With nnz == d every dot on such a row
is inf or NaN in any summation order, but WHICH one depends on the order
once finite partial sums overflow (+-3e38 next to an inf): the 4-chain dot
alone missed 2 of 776 such rows at d=5, so the dense bindings rescore
non-finite rows in strict order (score_extended_dense_nonfinite_rows).
"""

import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine
from isolation_forest_amd.utils.det_math import bf16_round
from isolation_forest_amd.utils.math import avg_path_length
from isolation_forest_amd.utils.params import ResolvedParams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MIN = np.float32(1.1754944e-38)
N_TRAIN = 4000
N_SCORE = 3001  # coprime with every tile size
MAX_BLOCKS = 8192  # launch cap of every scoring binding


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


_FUZZ = None


def _fuzz():
    """tools/fuzz_parity.py as a module (no side effects on import)."""
    global _FUZZ
    if _FUZZ is None:
        spec = importlib.util.spec_from_file_location(
            "ifa_fuzz_parity", os.path.join(REPO, "tools", "fuzz_parity.py"))
        _FUZZ = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_FUZZ)
    return _FUZZ


# ---------------------------------------------------------------------------
# B. edge-value data
# ---------------------------------------------------------------------------


def _from_bits(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


# +0, smallest f32 denormal, a mid denormal, the largest denormal, FLT_MIN,
# 1, then three denormals that are exact in bf16 (smallest, mid, largest)
# so the bf16 variants keep denormal cells after the round trip
_EDGE_POS = np.concatenate([
    np.array([0.0, 1e-45, 3e-41, 1.1754942e-38, 1.1754944e-38, 1.0],
             dtype=np.float32),
    _from_bits([0x00010000, 0x00400000, 0x007F0000]),
])
_EDGE = np.concatenate([_EDGE_POS, -_EDGE_POS])
_N_COPY = 4  # extra draw slots that copy another cell of the same column
_NONFINITE = np.array([np.inf, -np.inf, np.nan, 3e38, -3e38],
                      dtype=np.float32)


def _bf16_exact(X):
    """f32 matrix rounded through torch.bfloat16 (what the kernel sees)."""
    return torch.from_numpy(X).to(torch.bfloat16).float().numpy()


def _finite_edges_raw(rs, N, d):
    X = rs.normal(size=(N, d)).astype(np.float32)
    base = X.copy()
    hit = rs.random_sample((N, d)) < 0.10
    pick = rs.randint(0, len(_EDGE) + _N_COPY, size=(N, d))
    src = rs.randint(0, N, size=(N, d))
    cols = np.broadcast_to(np.arange(d), (N, d))
    repl = np.where(pick < len(_EDGE),
                    _EDGE[np.minimum(pick, len(_EDGE) - 1)],
                    base[src, cols])
    X[hit] = repl[hit]
    return X


def finite_edges(N, d, seed, bf16=False):
    X = _finite_edges_raw(np.random.RandomState(seed), N, d)
    return _bf16_exact(X) if bf16 else X


def all_denormal(N, d, seed, bf16=False):
    """Every value zero or denormal. bf16 keeps 7 mantissa bits, so its
    scale is larger (values are multiples of 2^-133 below 2^-126)."""
    rs = np.random.RandomState(seed)
    scale = 2.0 ** -129 if bf16 else 2.0 ** -135
    X = (rs.normal(size=(N, d)) * scale).astype(np.float32)
    X = _bf16_exact(X) if bf16 else X
    assert (np.abs(X) < FLT_MIN).all() and (X != 0).mean() > 0.9
    return X


def scoring_edges(N, d, seed, bf16=False):
    rs = np.random.RandomState(seed)
    X = _finite_edges_raw(rs, N, d)
    hit = rs.random_sample((N, d)) < 0.10
    pick = rs.randint(0, len(_NONFINITE), size=(N, d))
    X[hit] = _NONFINITE[pick][hit]
    return _bf16_exact(X) if bf16 else X


_GEN = {"finite_edges": finite_edges, "all_denormal": all_denormal,
        "scoring_edges": scoring_edges}
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _data(kind, N, d, bf16, seed):
    X = _memo(("data", kind, N, d, bf16, seed),
              lambda: _GEN[kind](N, d, seed, bf16))
    X.setflags(write=False)
    return X


def _train(kind, d, bf16, rows=N_TRAIN):
    return _data(kind, rows, d, bf16, 1000 + d)


def _subset(name, X, mask):
    """Memoised row subset of a memoised matrix (kept alive, read-only)."""
    def make():
        sub = np.ascontiguousarray(X[mask])
        sub.setflags(write=False)
        return sub
    return _memo(("subset", name, id(X)), make)


def _score_rows(kind, d, bf16):
    X = _data(kind, N_SCORE, d, bf16, 2000 + d)
    if kind == "scoring_edges":
        nonfinite = (~np.isfinite(X)).any(axis=1).sum()
        assert nonfinite >= 100, nonfinite
    if kind in ("scoring_edges", "finite_edges"):
        den = ((X != 0) & (np.abs(X) < FLT_MIN)).any(axis=1).sum()
        assert den >= 100, den
    return X


def _to_dev(X, bf16, dev):
    t = torch.from_numpy(np.array(X))  # copy: the memoised X is read-only
    if bf16:
        t = t.to(torch.bfloat16)  # exact: X is already bf16-rounded
    return t.to(dev)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------
# forests (CPU-built) and oracles, shared between tests
# ---------------------------------------------------------------------------


def _bags(n, d, k, T, seed, rows=N_TRAIN):
    bag = cpu_engine.sample_bags(rows, T, n, seed=seed, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, k, T, seed=seed)
    return bag, fs


def _depth_ok(forest):
    live = forest.feature >= -1
    depth = gpu_engine._node_depths(forest.feature, forest.right)
    return int(depth[live].max()) >= 5


def _tiny_threshold(forest):
    v = forest.value[forest.feature >= 0]
    return bool((np.abs(v) < FLT_MIN).any())


def _std_case(kind, n, d, k, T, bf16, rows=N_TRAIN):
    """(forest, bag, feature subsets, seed) of a CPU-built standard forest
    that reaches depth 5 and has a threshold that is denormal or zero, so
    the key transforms and the device packers see the values this file is
    about. Such a split needs a node whose rows are all tiny in the chosen
    feature, which most seeds do not produce on finite_edges: take the
    first seed that does."""
    def make():
        X = _train(kind, d, bf16, rows)
        for seed in range(17, 17 + 64):
            bag, fs = _bags(n, d, k, T, seed, rows)
            f = cpu_engine.build_forest(X, bag, fs, seed, n, k, d)
            if _depth_ok(f) and _tiny_threshold(f):
                return f, bag, fs, seed
        raise AssertionError("no seed gives a denormal or zero threshold")
    return _memo(("std", kind, n, d, k, T, bf16, rows), make)


def _std_forest(kind, n, d, k, T, bf16, rows=N_TRAIN):
    return _std_case(kind, n, d, k, T, bf16, rows)[0]


def _eif_forest(kind, n, d, T, ext, bf16, seed=17):
    def make():
        X = _train(kind, d, bf16)
        bag, fs = _bags(n, d, d, T, seed)
        f = cpu_engine.build_extended_forest(X, bag, fs, seed, n, d, d, ext)
        assert _depth_ok(f)
        assert np.isfinite(f.value).all() and np.isfinite(f.hyper_w).all()
        return f
    return _memo(("eif", kind, n, d, T, ext, bf16, seed), make)


def _bf16_weight_oracle(forest):
    f_b = copy.copy(forest)
    f_b.hyper_w = bf16_round(forest.hyper_w)
    return f_b


def _oracle(forest, X):
    def make():
        with np.errstate(all="ignore"):
            if hasattr(forest, "hyper_w"):
                ps = cpu_engine.path_lengths_extended(forest, X)
            else:
                ps = cpu_engine.path_lengths(forest, X)
        return forest, X, ps  # keeps both alive, so the ids stay unique
    # keyed by identity: forests and data are memoised and never mutated
    return _memo(("oracle", id(forest), id(X)), make)[2]


def _c(forest):
    return float(avg_path_length(forest.num_samples))


# ---------------------------------------------------------------------------
# A. kernel pinning
# ---------------------------------------------------------------------------


class Shell:
    """What the engine needs of a model: the forest and a pack cache."""

    def __init__(self, forest):
        self.forest = forest
        self._gpu_forest_cache = {}


class _Spy:
    """Recording proxy of the HIP extension: which bindings the router
    called, and the shapes they were given."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def wrapped(*args, **kwargs):
            shapes = [tuple(a.shape) for a in args
                      if isinstance(a, torch.Tensor)]
            self.calls.append((name, shapes))
            return fn(*args, **kwargs)
        return wrapped


def _routed(fn, shell, Xt, expect, finalize=False):
    """Score through the public router and assert the binding it chose.
    Returns (output, tensor shapes the binding received)."""
    from isolation_forest_amd.ops import load_extension

    spy = _Spy(load_extension())
    saved = gpu_engine.load_extension
    gpu_engine.load_extension = lambda: spy
    try:
        out = fn(shell, Xt, finalize=finalize)
    finally:
        gpu_engine.load_extension = saved
    assert [c[0] for c in spy.calls] == [expect], spy.calls
    return out, spy.calls[0][1]


def _v4_config(d, mn, bf16):
    """The (rpt, ilp, rows_lds, nodes_lds) instantiation the score_forest
    binding picks (mirror of its LDS config search and env switches)."""
    ilp_env = 8 if os.environ.get("IFA_SCORE_ILP", "").strip() == "8" else 4
    elem = 2 if bf16 else 4
    dpad = d + 1
    while (dpad % 4 != 2) if bf16 else (dpad % 2 != 1):
        dpad += 1
    nodes_lds = 2 * mn * 8 + 256 * dpad * elem <= 150 * 1024
    best = None
    for rpt, ilp in ((2, ilp_env), (1, ilp_env), (2, 2), (1, 2)):
        lds = (ilp * mn * 8 if nodes_lds else 0) + rpt * 256 * dpad * elem
        if lds > 150 * 1024:
            continue
        cand = (min(160 * 1024 // max(lds, 1), 3), rpt * ilp)
        if best is None or cand > best[0]:
            best = (cand, rpt, ilp)
    rows_lds = best is not None
    rpt, ilp = (best[1], best[2]) if rows_lds else (1, ilp_env)
    force = os.environ.get("IFA_SCORE_FORCE_GLOBAL")
    if force and int(force):
        rows_lds, rpt = False, 1
    return {"rpt": rpt, "ilp": ilp, "rows_lds": rows_lds,
            "nodes_lds": nodes_lds}


def _dense_D(d):
    for D in (8, 16, 32, 64):
        if d <= D:
            return D
    return 128


def _old_dense_predicate(forest, d):
    """score_extended_forest binding: old dense kernel vs general."""
    mn = forest.feature.shape[1]
    return forest.nnz == d and d % 4 == 0 and mn * 8 <= 120 * 1024


def _score_std(shell, Xt, finalize=False):
    assert gpu_engine._packed_fits(shell.forest, int(Xt.shape[1]))
    out, _ = _routed(gpu_engine.score_forest, shell, Xt, "score_forest",
                     finalize)
    return out


def _score_std_wide(shell, Xt, finalize=False):
    from isolation_forest_amd.ops import load_extension

    bf16 = Xt.dtype == torch.bfloat16
    aos, _, ex = gpu_engine._device_forest(shell, Xt.device,
                                           v4_key=("wide", bf16))
    assert aos.shape[2] == 4
    return load_extension().score_forest_wide(
        Xt, aos, ex["height"], _c(shell.forest), finalize)


def _score_eif(expect):
    def run(shell, Xt, finalize=False):
        out, shapes = _routed(gpu_engine.score_extended_forest, shell, Xt,
                              expect, finalize)
        f, d = shell.forest, int(Xt.shape[1])
        mn = f.feature.shape[1]
        if expect == "score_extended_sparse_v2":
            # X, nodes, values, hidx, hw, ncount: the NNZ template
            assert shapes[3] == (f.num_trees, mn, f.nnz)
        elif expect == "score_extended_dense_v2":
            assert shapes[3] == (f.num_trees, mn, _dense_D(d))
        elif expect == "score_extended_dense_v3":
            assert shapes[3] == (f.num_trees, mn, _dense_D(d) // 2)
        return out
    return run


def _score_eif_direct(old_dense):
    """The score_extended_forest binding, called with the engine's own
    pack: general strict-order kernel, or the old dense kernel."""
    def run(shell, Xt, finalize=False):
        from isolation_forest_amd.ops import load_extension

        f = shell.forest
        assert _old_dense_predicate(f, int(Xt.shape[1])) == old_dense
        aos, nc, ex = gpu_engine._device_forest(shell, Xt.device)
        return load_extension().score_extended_forest(
            Xt, aos, ex["hidx"], ex["hw"], nc, _c(f), finalize)
    return run


def _score_eif_dense_v2_direct(shell, Xt, finalize=False):
    """The dense v2 binding with the engine's own densified pack, for
    shapes the router sends elsewhere (nnz <= 5 goes to sparse v2)."""
    from isolation_forest_amd.ops import load_extension

    f, D = shell.forest, _dense_D(int(Xt.shape[1]))
    aos, nc, ex = gpu_engine._device_forest(shell, Xt.device,
                                            v4_key=("eif_dense", D))
    assert ex["hw"].shape == (f.num_trees, f.feature.shape[1], D)
    return load_extension().score_extended_dense_v2(
        Xt, aos, ex["values"], ex["hw"], nc, ex["height"], _c(f), finalize)


def _score_eif_wide(shell, Xt, finalize=False):
    from isolation_forest_amd.ops import load_extension

    aos, _, ex = gpu_engine._device_forest(shell, Xt.device,
                                           v4_key="eif_wide")
    assert aos.shape[2] == 4
    return load_extension().score_extended_wide(
        Xt, aos, ex["hidx"], ex["hw"], _c(shell.forest), finalize)


def _assert_bitwise(gpu_ps, cpu_ps, what):
    g, c = _bits(gpu_ps), _bits(cpu_ps)
    bad = np.nonzero(g != c)[0]
    assert len(bad) == 0, (
        f"{what}: {len(bad)}/{len(c)} rows differ from the oracle, first "
        f"row {int(bad[0])}: gpu {gpu_ps[bad[0]]} cpu {cpu_ps[bad[0]]}")


def _assert_dense_contract(gpu_ps, cpu_ps, oracle_forest, X, what):
    gpu_ps = gpu_ps.cpu().numpy()
    nonfinite = (~np.isfinite(X)).any(axis=1)
    nf_bad = np.nonzero(nonfinite & (_bits(gpu_ps) != _bits(cpu_ps)))[0]
    diff = np.abs(gpu_ps - cpu_ps)
    bad = np.nonzero(diff > 1e-3)[0]
    print(f"[dense] {what}: {len(bad)}/{len(X)} rows differ by > 1e-3; "
          f"{len(nf_bad)}/{int(nonfinite.sum())} non-finite rows not bitwise")
    assert len(nf_bad) == 0, (what, nf_bad[:8], diff[nf_bad[:8]])
    assert len(bad) <= 3, (what, bad[:8], diff[bad[:8]])
    with np.errstate(all="ignore"):
        for r in bad:
            assert _fuzz()._knife_edge_explained(oracle_forest, X[r]), (
                what, int(r), float(diff[r]))


# ---------------------------------------------------------------------------
# C1. build kernels on edge values
# ---------------------------------------------------------------------------


class TestBuildEdgeValues:
    """GPU-built forests are bit-identical to the CPU oracle's on data made
    of zeros, denormals, FLT_MIN and exact duplicates (same field list as
    test_gpu.py::TestStructuralParity)."""

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("kind", ["finite_edges", "all_denormal"])
    @pytest.mark.parametrize("n,d,k,T", [(128, 6, 6, 8), (64, 5, 3, 4)])
    def test_standard_build_identical(self, dev, n, d, k, T, kind, bf16):
        X = _train(kind, d, bf16)
        cpu_f, bag, fs, seed = _std_case(kind, n, d, k, T, bf16)
        assert _depth_ok(cpu_f) and _tiny_threshold(cpu_f)
        rp = ResolvedParams(num_samples=n, num_features=k,
                            total_rows=N_TRAIN, total_features=d)
        gpu_f = gpu_engine.build_forest(_to_dev(X, bf16, dev), bag, fs,
                                        seed, rp)
        for name in ["node_count", "feature", "right", "num_instances"]:
            np.testing.assert_array_equal(getattr(gpu_f, name),
                                          getattr(cpu_f, name), err_msg=name)
        np.testing.assert_array_equal(_bits(gpu_f.value), _bits(cpu_f.value))

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("kind", ["finite_edges", "all_denormal"])
    @pytest.mark.parametrize("ext_level", [0, 2, 5])
    def test_extended_build_identical(self, dev, ext_level, kind, bf16):
        n, d, T = 128, 6, 8
        X = _train(kind, d, bf16)
        bag, fs = _bags(n, d, d, T, 4)
        cpu_f = cpu_engine.build_extended_forest(X, bag, fs, 4, n, d, d,
                                                 ext_level)
        assert _depth_ok(cpu_f)
        rp = ResolvedParams(num_samples=n, num_features=d,
                            total_rows=N_TRAIN, total_features=d,
                            extension_level=ext_level)
        gpu_f = gpu_engine.build_extended_forest(_to_dev(X, bf16, dev), bag,
                                                 fs, 4, rp)
        for name in ["node_count", "feature", "right", "num_instances",
                     "hyper_idx"]:
            np.testing.assert_array_equal(getattr(gpu_f, name),
                                          getattr(cpu_f, name), err_msg=name)
        for name in ["hyper_w", "value"]:
            np.testing.assert_array_equal(_bits(getattr(gpu_f, name)),
                                          _bits(getattr(cpu_f, name)),
                                          err_msg=name)
        np.testing.assert_array_equal(gpu_f.offset64.view(np.int64),
                                      cpu_f.offset64.view(np.int64))

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_bag_gather_bitwise(self, dev, bf16):
        """Gathered rows keep NaN payloads, -0 and denormals bit for bit."""
        from isolation_forest_amd.ops import load_extension

        X = _score_rows("scoring_edges", 6, bf16)
        idx = cpu_engine.sample_bags(N_SCORE, 10, 64, seed=1,
                                     bootstrap=False)
        bags = load_extension().bag_gather(
            _to_dev(X, bf16, dev), torch.from_numpy(idx).to(dev))
        np.testing.assert_array_equal(_bits(bags), _bits(X[idx]))


# ---------------------------------------------------------------------------
# C2. every route on edge values
# ---------------------------------------------------------------------------


def _score_sets(d, bf16):
    return [("scoring_edges", _score_rows("scoring_edges", d, bf16)),
            ("all_denormal", _score_rows("all_denormal", d, bf16))]


class TestScoreEdgeValues:
    """Forests built on finite_edges score scoring_edges (and, on the
    bitwise routes, all_denormal rows) through each named kernel."""

    def _bitwise(self, dev, forest, score, d, bf16, what, sets=None):
        shell = Shell(forest)
        for kind, X in (sets or _score_sets(d, bf16)):
            gpu_ps = score(shell, _to_dev(X, bf16, dev))
            _assert_bitwise(gpu_ps.cpu().numpy(), _oracle(forest, X),
                            f"{what} on {kind}")

    # --- standard forests -------------------------------------------------

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("switch", ["lds", "ilp8", "glob"])
    def test_standard_v4(self, dev, monkeypatch, switch, bf16):
        """S-lds / S-ilp8 / S-glob."""
        if switch == "ilp8":
            monkeypatch.setenv("IFA_SCORE_ILP", "8")
        elif switch == "glob":
            monkeypatch.setenv("IFA_SCORE_FORCE_GLOBAL", "1")
        d = 6
        for kind in ("finite_edges", "all_denormal"):
            forest = _std_forest(kind, 128, d, d, 8, bf16)
            cfg = _v4_config(d, forest.feature.shape[1], bf16)
            assert cfg["nodes_lds"]
            assert cfg["rows_lds"] == (switch != "glob")
            assert cfg["ilp"] == (8 if switch == "ilp8" else 4)
            sets = (None if kind == "finite_edges" else
                    [("all_denormal", _score_rows("all_denormal", d, bf16))])
            self._bitwise(dev, forest, _score_std, d, bf16,
                          f"S-{switch} ({kind} forest)", sets)

    @pytest.mark.parametrize("n,nodes_lds,ilp", [(4096, True, 2),
                                                 (8192, False, 4)])
    def test_standard_v4_deep(self, dev, n, nodes_lds, ilp):
        """S-deep. At n=4096 (8191 nodes/tree) the binding still stages
        nodes in LDS, two trees at a time (the ILP=2 fallback); n=8192 is
        the smallest power of two whose trees leave LDS (NODES_LDS=false).
        """
        d, bf16 = 6, False
        forest = _std_forest("finite_edges", n, d, d, 4, bf16, rows=9000)
        cfg = _v4_config(d, forest.feature.shape[1], bf16)
        assert cfg["nodes_lds"] == nodes_lds and cfg["ilp"] == ilp
        assert cfg["rows_lds"]
        self._bitwise(dev, forest, _score_std, d, bf16, f"S-deep n={n}")

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_standard_wide_direct(self, dev, bf16):
        """S-wide."""
        d = 6
        forest = _std_forest("finite_edges", 128, d, d, 8, bf16)
        self._bitwise(dev, forest, _score_std_wide, d, bf16, "S-wide")

    # --- extended forests, bitwise routes -----------------------------------

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_eif0_v4(self, dev, bf16):
        """E-0: ext-0 forests walk the standard v4 kernel for NaN-free
        rows; a batch holding a NaN takes the strict-order sparse kernel.
        Both must be bitwise."""
        d = 6
        forest = _eif_forest("finite_edges", 128, d, 8, 0, bf16)
        assert gpu_engine._eif0_eligible(forest, d)
        X = _score_rows("scoring_edges", d, bf16)
        no_nan = _subset("no_nan", X, ~np.isnan(X).any(axis=1))
        assert np.isinf(no_nan).any(axis=1).sum() >= 100
        cfg = _v4_config(d, forest.feature.shape[1], bf16)
        assert cfg["rows_lds"] and cfg["nodes_lds"]
        self._bitwise(
            dev, forest, _score_std_as_eif0, d, bf16, "E-0",
            [("scoring_edges without NaN rows", no_nan),
             ("all_denormal", _score_rows("all_denormal", d, bf16))])
        self._bitwise(dev, forest, _score_eif("score_extended_sparse_v2"),
                      d, bf16, "E-0 NaN fallback", [("scoring_edges", X)])

    @pytest.mark.parametrize("nnz,bf16", [
        (1, False), (2, False), (2, True), (3, False), (4, False),
        (5, False), (5, True)])
    def test_sparse_v2(self, dev, monkeypatch, nnz, bf16):
        """E-sp1..5 (nnz=1 needs IFA_EIF0_SPARSE=1 to leave the v4 walk)."""
        if nnz == 1:
            monkeypatch.setenv("IFA_EIF0_SPARSE", "1")
        d = 7
        score = _score_eif("score_extended_sparse_v2")
        forest = _eif_forest("finite_edges", 128, d, 8, nnz - 1, bf16)
        assert forest.nnz == nnz
        self._bitwise(dev, forest, score, d, bf16, f"E-sp{nnz}")
        forest = _eif_forest("all_denormal", 128, d, 8, nnz - 1, bf16)
        self._bitwise(dev, forest, score, d, bf16,
                      f"E-sp{nnz} (all_denormal forest)",
                      [("all_denormal", _score_rows("all_denormal", d, bf16))])

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("nnz", [3, 7])
    def test_general_direct(self, dev, nnz, bf16):
        """E-gen."""
        d = 7
        forest = _eif_forest("finite_edges", 128, d, 8, nnz - 1, bf16)
        self._bitwise(dev, forest, _score_eif_direct(False), d, bf16,
                      f"E-gen nnz={nnz}")

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_extended_wide_direct(self, dev, bf16):
        """E-ewide."""
        d = 7
        forest = _eif_forest("finite_edges", 128, d, 8, 2, bf16)
        self._bitwise(dev, forest, _score_eif_wide, d, bf16, "E-ewide")

    # --- extended forests, dense routes -------------------------------------

    @pytest.mark.parametrize("d,D", [(5, 8), (7, 8), (13, 16), (31, 32),
                                     (40, 64)])
    def test_dense_v2(self, dev, d, D):
        """E-d2: f32 rows, nnz == d, d < D padding. The router keeps
        nnz <= 5 on sparse v2, so d=5 calls the binding directly. d=5 is
        the case that needs the strict-order pass for non-finite rows:
        rows like [3e38, .48, -.30, -inf, 3e38] gave NaN in the 4-chain dot
        and -inf in the oracle's order (path sums 2.0 apart)."""
        assert _dense_D(d) == D
        forest = _eif_forest("finite_edges", 128, d, 8, d - 1, False)
        score = (_score_eif_dense_v2_direct if d <= 5
                 else _score_eif("score_extended_dense_v2"))
        shell = Shell(forest)
        for kind in ("scoring_edges", "finite_edges"):
            X = _score_rows(kind, d, False)
            gpu_ps = score(shell, _to_dev(X, False, dev))
            _assert_dense_contract(gpu_ps, _oracle(forest, X), forest, X,
                                   f"E-d2 d={d} on {kind}")

    @pytest.mark.parametrize("d,rpt2", [(7, False), (13, False), (31, False),
                                        (31, True), (47, False),
                                        (100, False)])
    def test_dense_v3(self, dev, monkeypatch, d, rpt2):
        """E-d3: bf16 rows, nnz == d, odd-d pair-packing tail; oracle with
        the same RNE-bf16 weights the kernel stages."""
        if rpt2:
            monkeypatch.setenv("IFA_EIF_V3_RPT2", "1")
            assert _dense_D(d) == 32  # the only D the switch changes
        forest = _eif_forest("finite_edges", 128, d, 8, d - 1, True)
        f_b = _memo(("bf16w", id(forest)),
                    lambda: _bf16_weight_oracle(forest))
        shell = Shell(forest)
        for kind in ("scoring_edges", "finite_edges"):
            X = _score_rows(kind, d, True)
            gpu_ps = _score_eif("score_extended_dense_v3")(
                shell, _to_dev(X, True, dev))
            _assert_dense_contract(
                gpu_ps, _oracle(f_b, X), f_b, X,
                f"E-d3 d={d}{' rpt2' if rpt2 else ''} on {kind}")

    @pytest.mark.parametrize("d,ext,bf16", [(12, 7, False), (12, 7, True),
                                            (40, 9, False)])
    def test_densified(self, dev, d, ext, bf16):
        """E-dz: 6 <= nnz < d. Finite rows take the densified dense kernel
        (unselected coordinates carry weight 0); a batch with a non-finite
        cell would compute 0*inf = NaN there, so it must take the general
        strict-order kernel and match the oracle bitwise."""
        forest = _eif_forest("finite_edges", 128, d, 8, ext, bf16)
        assert 6 <= forest.nnz < d
        X = _score_rows("scoring_edges", d, bf16)
        what = f"E-dz d={d} ext={ext} {'bf16' if bf16 else 'f32'}"

        finite = _subset("finite", X, np.isfinite(X).all(axis=1))
        assert len(finite) >= 30 and (np.abs(finite) > 1e38).any()
        kernel = ("score_extended_dense_v3" if bf16
                  else "score_extended_dense_v2")
        oracle_f = forest
        if bf16:
            oracle_f = _memo(("bf16w", id(forest)),
                             lambda: _bf16_weight_oracle(forest))
        shell = Shell(forest)
        for kind, Xf in (("finite rows of scoring_edges", finite),
                         ("finite_edges", _score_rows("finite_edges", d,
                                                      bf16))):
            gpu_ps = _score_eif(kernel)(shell, _to_dev(Xf, bf16, dev))
            _assert_dense_contract(gpu_ps, _oracle(oracle_f, Xf), oracle_f,
                                   Xf, f"{what} on {kind}")

        gpu_ps = _score_eif("score_extended_forest")(
            Shell(forest), _to_dev(X, bf16, dev))
        cpu_ps = _oracle(forest, X)
        _assert_dense_contract(gpu_ps, cpu_ps, forest, X, what)
        _assert_bitwise(gpu_ps.cpu().numpy(), cpu_ps, what)

    # --- GPU-built forests: the device packers ------------------------------

    def _gpu_built(self, dev, d, bf16, ext_level):
        n, T = 128, 8
        X = _train("finite_edges", d, bf16)
        if ext_level is None:
            # the seed whose CPU twin has a denormal or zero threshold
            _, bag, fs, seed = _std_case("finite_edges", n, d, d, T, bf16)
        else:
            seed = 23
            bag, fs = _bags(n, d, d, T, seed)
        rp = ResolvedParams(num_samples=n, num_features=d,
                            total_rows=N_TRAIN, total_features=d,
                            extension_level=ext_level or 0)
        build = (gpu_engine.build_forest if ext_level is None
                 else gpu_engine.build_extended_forest)
        forest = build(_to_dev(X, bf16, dev), bag, fs, seed, rp)
        assert _depth_ok(forest)
        assert forest._device_raw["device"] == str(dev)
        return forest

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_gpu_built_standard(self, dev, bf16):
        """S-lds with thresholds packed on device (_key32_dev /
        _bf16_threshold_keys_dev) from denormal and zero split values."""
        d = 6
        forest = self._gpu_built(dev, d, bf16, None)
        assert _tiny_threshold(forest)
        aos_d, nc_d, h_d = gpu_engine._nodes_packed_v4_device(
            forest._device_raw, forest.num_trees, d, bf16)
        aos_h, nc_h, h_h = gpu_engine._nodes_packed_v4(forest, d, bf16)
        np.testing.assert_array_equal(aos_d.cpu().numpy(), aos_h)
        np.testing.assert_array_equal(nc_d.cpu().numpy(), nc_h)
        assert h_d == h_h
        self._bitwise(dev, forest, _score_std, d, bf16, "S-lds GPU-built")

    @pytest.mark.parametrize("ext_level,kernel", [
        (0, "score_forest"), (1, "score_extended_sparse_v2")])
    def test_gpu_built_extended(self, dev, ext_level, kernel):
        """E-0 and E-sp2 on GPU-built forests (_eif_nodes_values_device)."""
        d, bf16 = 6 if ext_level == 0 else 7, False
        forest = self._gpu_built(dev, d, bf16, ext_level)
        aos_d, val_d, _, h_d = gpu_engine._eif_nodes_values_device(
            forest._device_raw)
        aos_h, val_h, h_h = gpu_engine._eif_nodes_values(forest)
        np.testing.assert_array_equal(aos_d.cpu().numpy(), aos_h)
        np.testing.assert_array_equal(_bits(val_d), _bits(val_h))
        assert h_d == h_h
        X = _score_rows("scoring_edges", d, bf16)
        sets = [("all_denormal", _score_rows("all_denormal", d, bf16))]
        if ext_level == 0:
            no_nan = X[~np.isnan(X).any(axis=1)]
            sets.append(("scoring_edges without NaN rows", no_nan))
        else:
            sets.append(("scoring_edges", X))
        shell = Shell(forest)
        for kind, Xs in sets:
            gpu_ps = _score_eif(kernel)(shell, _to_dev(Xs, bf16, dev))
            with np.errstate(all="ignore"):
                cpu_ps = cpu_engine.path_lengths_extended(forest, Xs)
            _assert_bitwise(gpu_ps.cpu().numpy(), cpu_ps,
                            f"GPU-built ext={ext_level} on {kind}")


def _score_std_as_eif0(shell, Xt, finalize=False):
    """ext-0 EIF through the router: must land on the standard v4 walk."""
    out, _ = _routed(gpu_engine.score_extended_forest, shell, Xt,
                     "score_forest", finalize)
    return out


# ---------------------------------------------------------------------------
# C3. a row's result depends only on that row
# ---------------------------------------------------------------------------

# route id -> (forest kind, d, nnz, bf16, scorer, env, R); R = the largest
# rows-per-block-iteration the kernel can pick
_POSITION_ROUTES = {
    "S-lds-f32": ("std", 6, None, False, _score_std, {}, 512),
    "S-lds-bf16": ("std", 6, None, True, _score_std, {}, 512),
    "S-glob": ("std", 6, None, False, _score_std,
               {"IFA_SCORE_FORCE_GLOBAL": "1"}, 512),
    "S-wide": ("std", 6, None, False, _score_std_wide, {}, 256),
    "E-sp2": ("eif", 7, 2, False, _score_eif("score_extended_sparse_v2"),
              {}, 512),
    "E-gen": ("eif", 7, 3, False, _score_eif_direct(False), {}, 256),
    "E-olddense": ("eif", 8, 8, False, _score_eif_direct(True), {}, 256),
    "E-d2": ("eif", 7, 7, False, _score_eif("score_extended_dense_v2"), {},
             1024),
    "E-d3": ("eif", 7, 7, True, _score_eif("score_extended_dense_v3"), {},
             1024),
    "E-ewide": ("eif", 7, 3, False, _score_eif_wide, {}, 256),
}
_PREFIXES = (1, 63, 64, 65, 255, 256, 257, 511, 513, 1025)


class TestRowPositionInvariance:
    """Scoring a prefix, or the same rows far into the grid-stride loop,
    gives each row the same bits. Oracle parity of score(X_small) is
    TestScoreEdgeValues' job."""

    def _setup(self, dev, monkeypatch, route):
        kind, d, nnz, bf16, score, env, R = _POSITION_ROUTES[route]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        n, T = 64, 4
        if kind == "std":
            forest = _std_forest("finite_edges", n, d, d, T, bf16)
            if score is _score_std:
                cfg = _v4_config(d, forest.feature.shape[1], bf16)
                assert cfg["rows_lds"] == (route != "S-glob")
                assert cfg["rpt"] * 256 <= R
        else:
            forest = _eif_forest("finite_edges", n, d, T, nnz - 1, bf16)
        X = _score_rows("finite_edges", d, bf16)
        Xt = _to_dev(X, bf16, dev)
        shell = Shell(forest)
        return shell, score, Xt, R

    @pytest.mark.parametrize("route", list(_POSITION_ROUTES))
    def test_prefixes(self, dev, monkeypatch, route):
        shell, score, Xt, _ = self._setup(dev, monkeypatch, route)
        full = score(shell, Xt).view(torch.int32)
        for m in _PREFIXES:
            part = score(shell, Xt[:m].contiguous()).view(torch.int32)
            assert part.shape == (m,)
            assert torch.equal(part, full[:m]), (route, m)

    @pytest.mark.parametrize("route", list(_POSITION_ROUTES))
    def test_grid_stride(self, dev, monkeypatch, route):
        shell, score, Xt, R = self._setup(dev, monkeypatch, route)
        n_big = MAX_BLOCKS * R + R + 77  # second iteration, ragged tail
        small = score(shell, Xt).view(torch.int32)
        reps = -(-n_big // N_SCORE)
        X_big = Xt.repeat(reps, 1)[:n_big].contiguous()
        big = score(shell, X_big).view(torch.int32)
        assert big.shape == (n_big,)
        expect = small.repeat(reps)[:n_big]
        assert torch.equal(big, expect), (
            route, int((big != expect).sum().item()))


# ---------------------------------------------------------------------------
# C4. finalized scores
# ---------------------------------------------------------------------------


class TestOutputContract:
    @pytest.mark.parametrize("route", ["S-lds", "E-sp2"])
    def test_finalized_scores_bitwise(self, dev, route):
        bf16 = False
        if route == "S-lds":
            d = 6
            forest = _std_forest("finite_edges", 128, d, d, 8, bf16)
            score = _score_std
        else:
            d = 7
            forest = _eif_forest("finite_edges", 128, d, 8, 1, bf16)
            score = _score_eif("score_extended_sparse_v2")
        X = _score_rows("scoring_edges", d, bf16)
        got = score(Shell(forest), _to_dev(X, bf16, dev),
                    finalize=True).cpu().numpy()
        want = cpu_engine.scores_from_path_sums(
            _oracle(forest, X), forest.num_trees, forest.num_samples)
        assert np.isfinite(got).all()
        assert (got > 0).all() and (got < 1).all()
        _assert_bitwise(got, want, f"{route} finalized scores")
