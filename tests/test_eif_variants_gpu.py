"""GPU tests (MI355X): every reachable staging variant of the two kernels
behind the score_extended_forest binding, and the dense EIF kernels held to
order-exact references, knife-edge rows included.

The case table, its forests, rows and references live in
tests/test_eif_variants_ref.py, which checks without a GPU that each case
reaches its variant and that the planted rows separate the summation
orders. Here each call is pinned to its kernel: router calls through the
recording proxy of tests/test_gpu_edges.py, direct binding calls with the
engine's own pack, and in both the mirror of the binding's LDS budget
(tests/eif_order_ref.py) names the template instance.

  general kernel   bitwise against cpu_engine.path_lengths_extended
  old dense        bitwise against walk_chain4("muladd")
  dense v2         bitwise against walk_chain4("fma", D); rows with an
                   inf / NaN cell are rescored in strict order by
                   score_extended_dense_nonfinite_rows and equal the oracle
  dense v3         keeps its tolerance contract (tests/test_gpu_edges.py):
                   the rounding inside v_dot2c_f32_bf16 is not specified
  finalize         every EIF kernel's own epilogue against
                   cpu_engine.scores_from_path_sums of its own path sums
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests import eif_order_ref as R  # noqa: E402
from tests import test_eif_variants_ref as C  # noqa: E402
from tests.test_gpu_edges import (  # noqa: E402
    Shell,
    _assert_bitwise,
    _assert_dense_contract,
    _c,
    _score_eif,
    _score_eif_dense_v2_direct,
    _score_eif_direct,
    _score_eif_wide,
    scoring_edges,
)
from tests.test_score_layout_gpu import _to_dev  # noqa: E402
from tests.test_strided_gpu import (  # noqa: E402
    _assert_handed,
    _recorded,
    _view,
)

N = C.N_SCORE
VIEW_LAYOUTS = ["pitched", "feature"]
BINDING = "score_extended_forest"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _shell(spec):
    return C.memo(("shell", spec), lambda: Shell(C.forest_of(spec)))


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------
# row sets
# ---------------------------------------------------------------------------


def _edge_rows(d, kind):
    """scoring_edges (NaN, +-inf, +-3e38, denormals) in the row dtype."""
    return C.memo(("edges", d, kind), lambda: _frozen(
        R.round_rows(scoring_edges(N, d, 4000 + d), kind)))


_NONFINITE = np.array([np.inf, -np.inf, np.nan, 3e38, -3e38],
                      dtype=np.float32)


def _nonfinite_rows(spec, d, kind):
    """The planted rows, a third of them with one to three cells replaced
    by inf, -inf, NaN or +-3e38 (which is inf in fp16)."""
    def make():
        rs = np.random.RandomState(6000 + d)
        X = np.array(C.planted_rows(spec, d, kind))
        for r in np.nonzero(rs.random_sample(N) < 1 / 3)[0]:
            cols = rs.randint(0, d, size=rs.randint(1, 4))
            X[r, cols] = _NONFINITE[rs.randint(0, 5, size=len(cols))]
        X = R.round_rows(X, kind)
        bad = (~np.isfinite(X)).any(axis=1).sum()
        assert 100 <= bad <= N - 100, bad
        return _frozen(X)
    return C.memo(("nonfinite", spec, d, kind), make)


def _view_rows(d, kind, zero_row=False):
    """Gaussian rows with a NaN and an inf in the columns a walk that reads
    X through the strides itself reaches last (>= 128 where d allows)."""
    def make():
        X = np.array(C.gauss_rows(d, kind, zero_row))
        lo = 128 if d > 129 else d - 2
        for k, r in enumerate((5, 255, 256, 1500, N - 1)):
            X[r, lo + k % (d - lo)] = np.nan if k % 2 == 0 else np.inf
        return _frozen(X)
    return C.memo(("viewrows", d, kind, zero_row), make)


def _run_view(dev, score, binding_of_call, X, kind, layout, want, what):
    """Score the packed rows and their view; the view must reach the
    binding where it lies, and both must give `want`, bit for bit."""
    packed = _to_dev(X, kind, dev)
    view = _view(packed, layout)
    got_p = score(packed)
    got_v, calls = _recorded(score, view)
    if binding_of_call is not None:  # through the router
        _assert_handed(calls, binding_of_call, view, layout)
    _assert_bitwise(got_p.cpu().numpy(), want, f"{what} packed")
    _assert_bitwise(got_v.cpu().numpy(), want, f"{what} {layout}")


# ---------------------------------------------------------------------------
# general kernel
# ---------------------------------------------------------------------------


def _general_scorer(case):
    spec, d, kind, via, want = C.GENERAL_CASES[case]
    f = C.forest_of(spec)
    assert R.general_variant(d, f.feature.shape[1], f.nnz,
                             R.ELEM[kind]) == want
    score = _score_eif(BINDING) if via == "router" else \
        _score_eif_direct(False)
    return spec, d, kind, via, score


def _rows_global_cases():
    return [c for c, v in C.GENERAL_CASES.items() if not v[4][0]]


class TestGeneralKernel:
    @pytest.mark.parametrize("case", list(C.GENERAL_CASES))
    def test_bitwise(self, dev, case):
        spec, d, kind, _, score = _general_scorer(case)
        complete = spec[0] == "complete"
        shell = _shell(spec)
        for name, X in (("gauss", C.gauss_rows(d, kind, zero_row=complete)),
                        ("edges", _edge_rows(d, kind)),
                        ("planted", C.planted_rows(spec, d, kind))):
            got = score(shell, _to_dev(X, kind, dev))
            _assert_bitwise(got.cpu().numpy(),
                            C.reference(spec, X, "oracle"),
                            f"general {case} on {name}")

    @pytest.mark.parametrize("layout", VIEW_LAYOUTS)
    @pytest.mark.parametrize("case", _rows_global_cases())
    def test_rows_global_views(self, dev, case, layout):
        """ROWS_LDS = false: the walk reads X through both strides."""
        spec, d, kind, via, _ = _general_scorer(case)
        shell = _shell(spec)
        X = _view_rows(d, kind, zero_row=spec[0] == "complete")
        want = C.reference(spec, X, "oracle")
        if via == "router":
            def score(Xt):
                return gpu_engine.score_extended_forest(shell, Xt,
                                                        finalize=False)
            binding = BINDING
        else:
            def score(Xt):
                Xin = gpu_engine._rows_in_place(Xt)
                assert Xin.data_ptr() == Xt.data_ptr()
                assert Xin.stride() == Xt.stride()
                return _score_eif_direct(False)(shell, Xin)
            binding = None
        _run_view(dev, score, binding, X, kind, layout, want,
                  f"general {case}")


# ---------------------------------------------------------------------------
# old dense kernel
# ---------------------------------------------------------------------------


def _old_dense_setup(case):
    d, kind = case
    spec = C.old_dense_spec(d)
    f = C.forest_of(spec)
    mn = f.feature.shape[1]
    assert R.takes_old_dense(d, mn, f.nnz)
    assert R.old_dense_variant(d, mn, R.ELEM[kind]) == C.OLD_DENSE_CASES[case]
    return spec, f


class TestOldDenseKernel:
    @pytest.mark.parametrize("case", list(C.OLD_DENSE_CASES), ids=C.dense_id)
    def test_bitwise_vs_muladd_chains(self, dev, case):
        d, kind = case
        spec, f = _old_dense_setup(case)
        shell, score = _shell(spec), _score_eif(BINDING)
        Xg = C.gauss_rows(d, kind)
        for name, X in (("gauss", Xg),
                        ("planted", C.planted_rows(spec, d, kind)),
                        ("nonfinite", _nonfinite_rows(spec, d, kind))):
            got = score(shell, _to_dev(X, kind, dev))
            _assert_bitwise(got.cpu().numpy(),
                            C.reference(spec, X, "muladd"),
                            f"old dense d={d} {kind} on {name}")
            if X is Xg:
                _assert_dense_contract(got, C.reference(spec, X, "oracle"),
                                       f, X, f"old dense d={d} {kind}")

    @pytest.mark.parametrize("layout", VIEW_LAYOUTS)
    @pytest.mark.parametrize(
        "case", [c for c, v in C.OLD_DENSE_CASES.items() if not v[0]],
        ids=C.dense_id)
    def test_rows_global_views(self, dev, case, layout):
        d, kind = case
        spec, _ = _old_dense_setup(case)
        shell = _shell(spec)
        X = _view_rows(d, kind)

        def score(Xt):
            return gpu_engine.score_extended_forest(shell, Xt,
                                                    finalize=False)
        _run_view(dev, score, BINDING, X, kind, layout,
                  C.reference(spec, X, "muladd"),
                  f"old dense d={d} {kind}")


# ---------------------------------------------------------------------------
# dense v2
# ---------------------------------------------------------------------------


def _v2_expected(spec, X, D):
    """fma chains; rows with an inf / NaN cell come from the strict-order
    rescoring pass and equal the oracle."""
    rescored = (~np.isfinite(X)).any(axis=1)
    return np.where(rescored, C.reference(spec, X, "oracle"),
                    C.reference(spec, X, "fma", D))


class TestDenseV2:
    @pytest.mark.parametrize("case", C.DENSE_V2_CASES, ids=C.dense_id)
    def test_bitwise_vs_fma_chains(self, dev, monkeypatch, case):
        d, D, kind = case
        if kind == "bf16":
            monkeypatch.setenv("IFA_EIF_DENSE_V2", "1")
        spec = C.dense_v2_spec(d)
        # the router keeps nnz <= 5 on sparse v2
        score = (_score_eif_dense_v2_direct if d <= 5
                 else _score_eif("score_extended_dense_v2"))
        shell = _shell(spec)
        for name, X in (("gauss", C.gauss_rows(d, kind)),
                        ("planted", C.planted_rows(spec, d, kind)),
                        ("nonfinite", _nonfinite_rows(spec, d, kind))):
            got = score(shell, _to_dev(X, kind, dev))
            _assert_bitwise(got.cpu().numpy(), _v2_expected(spec, X, D),
                            f"dense v2 d={d} D={D} {kind} on {name}")

    def test_densified(self, dev):
        """6 <= nnz < d: unselected coordinates carry weight 0 and their
        products join the chains like any other term (finite rows only;
        others take the general kernel, tests/test_gpu_edges.py)."""
        d, _, D = C.DENSIFIED_V2
        spec = C.densified_spec()
        shell, score = _shell(spec), _score_eif("score_extended_dense_v2")
        for name, X in (("gauss", C.gauss_rows(d, "f32")),
                        ("planted", C.planted_rows(spec, d, "f32"))):
            got = score(shell, _to_dev(X, "f32", dev))
            _assert_bitwise(got.cpu().numpy(),
                            C.reference(spec, X, "fma", D),
                            f"densified v2 d={d} on {name}")


# ---------------------------------------------------------------------------
# finalize epilogues
# ---------------------------------------------------------------------------

# name -> (forest spec, d, kind, scorer, rows, env)
_V2_SPEC, _V3_SPEC = C.dense_v2_spec(13), C.dense_v2_spec(13)
_FINALIZE = {
    "general-TTT": (C.GENERAL_CASES["rows-f32-d132"][0], 132, "f32",
                    _score_eif(BINDING), "gauss"),
    "general-FFF": (C.GENERAL_CASES["highid-f32-d144"][0], 144, "f32",
                    _score_eif(BINDING), "gauss"),
    "old-dense": (C.old_dense_spec(72), 72, "f32", _score_eif(BINDING),
                  "gauss"),
    "dense-v2": (_V2_SPEC, 13, "f32", _score_eif("score_extended_dense_v2"),
                 "gauss"),
    "dense-v3": (_V3_SPEC, 13, "bf16", _score_eif("score_extended_dense_v3"),
                 "gauss"),
    # rows with an inf / NaN cell are written by the rescoring kernel's own
    # epilogue, the others by the dense kernel's
    "nonfinite-rows-v2": (_V2_SPEC, 13, "f32",
                          _score_eif("score_extended_dense_v2"), "nonfinite"),
    "nonfinite-rows-v3": (_V3_SPEC, 13, "bf16",
                          _score_eif("score_extended_dense_v3"), "nonfinite"),
    "wide": (C.GENERAL_CASES["hyper-nnz5"][0], 7, "f32", _score_eif_wide,
             "gauss"),
}


class TestFinalizeEpilogues:
    @pytest.mark.parametrize("route", list(_FINALIZE))
    def test_bitwise_vs_cpu_formula(self, dev, route):
        """finalize=True equals scores_from_path_sums of the SAME kernel's
        finalize=False output: the epilogue alone, whatever the dot."""
        spec, d, kind, score, rows = _FINALIZE[route]
        f, shell = C.forest_of(spec), _shell(spec)
        if route == "general-TTT":
            assert C.GENERAL_CASES["rows-f32-d132"][4] == (True,) * 3
        if route == "general-FFF":
            assert C.GENERAL_CASES["highid-f32-d144"][4] == (False,) * 3
        X = (C.gauss_rows(d, kind) if rows == "gauss"
             else _nonfinite_rows(spec, d, kind))
        Xt = _to_dev(X, kind, dev)
        raw = score(shell, Xt, finalize=False).cpu().numpy()
        got = score(shell, Xt, finalize=True).cpu().numpy()
        assert np.isfinite(raw).all() and len(np.unique(raw)) > N // 4
        want = cpu_engine.scores_from_path_sums(raw, f.num_trees,
                                                f.num_samples)
        assert np.isfinite(got).all()
        assert (got > 0).all() and (got < 1).all()
        _assert_bitwise(got, want, f"{route} finalize epilogue")
        assert _c(f) == R.c_norm(f)
