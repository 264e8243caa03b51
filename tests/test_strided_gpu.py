"""GPU tests (MI355X) for input layouts: every kernel that reads X takes the
view's two element strides, so pitched row-major views (column slices of a
wider table, row sub-sampling) and feature-major views (a [d, N] buffer seen
through .T) are scored, fitted and explained where they lie, with the bits
of the same call on the packed copy. Views with both strides != 1 still go
through one .contiguous() copy.

Every view is laid over a base buffer filled with NaN, so a read outside the
view changes a walk. A recording proxy of the extension shows which binding
ran and which tensor it was handed: for an in-place layout that tensor has
the view's data pointer and strides (this is what fails when the engine
copies), for the fallback it is packed.

Oracle for the bitwise routes: the strict-order CPU engine, as in
tests/test_score_layout_gpu.py. The tolerance routes (dense v2/v3) are
compared with the same kernel on the packed copy only, which is bitwise
because the kernels are deterministic and the layout changes loads alone.
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
from tests.test_gpu_edges import (  # noqa: E402
    MAX_BLOCKS,
    Shell,
    _assert_bitwise,
)
from tests.test_score_layout_gpu import (  # noqa: E402
    _forest,
    _round,
    _rows,
    _to_dev,
)

KINDS = ["bf16", "f16", "f32"]
IN_PLACE = ["pitched", "pitched16", "rowstep", "feature"]
LAYOUTS = IN_PLACE + ["fallback"]
N_ROWS = 777  # one full 512-row tile and a tail; crosses rows 127/128, 255/256

_MEMO = {}  # this file's own fixtures (shells, references, fitted models)


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------


def _odd(x):
    return x | 1


def _view(Xd, layout):
    """Xd's values seen through `layout`, over a NaN-filled base buffer."""
    N, d = Xd.shape

    def base(*shape):
        return torch.full(shape, float("nan"), dtype=Xd.dtype,
                          device=Xd.device)
    if layout == "pitched":  # odd pitch, odd offsets: misaligned row starts
        v = base(N + 5, _odd(d + 11))[2:2 + N, 3:3 + d]
    elif layout == "pitched16":  # row starts stay 16-byte aligned
        assert d % 8 == 0
        v = base(N + 3, d + 16)[1:1 + N, 8:8 + d]
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 0
    elif layout == "rowstep":
        v = base(2 * N, d)[::2]
    elif layout == "feature":
        v = base(d + 2, N + 7)[1:1 + d, 4:4 + N].T
    elif layout == "fallback":
        v = base(N, 2 * d)[:, ::2]
    else:
        raise KeyError(layout)
    v.copy_(Xd)
    ibits = torch.int32 if Xd.element_size() == 4 else torch.int16
    assert v.shape == Xd.shape
    assert torch.equal(v.contiguous().view(ibits), Xd.view(ibits))
    return v


def _layouts_for(d, layouts=LAYOUTS):
    return [lo for lo in layouts if lo != "pitched16" or d % 8 == 0]


# ---------------------------------------------------------------------------
# recording proxy of the extension
# ---------------------------------------------------------------------------


class _Recorder:
    """Which bindings ran, and the X each was handed (kept alive, so its
    data pointer cannot be recycled before the assertion)."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def wrapped(*args, **kwargs):
            self.calls.append((name, args[0]))
            return fn(*args, **kwargs)
        return wrapped


def _recorded(fn, *args, **kwargs):
    from isolation_forest_amd.ops import load_extension

    rec = _Recorder(load_extension())
    saved = gpu_engine.load_extension
    gpu_engine.load_extension = lambda: rec
    try:
        out = fn(*args, **kwargs)
    finally:
        gpu_engine.load_extension = saved
    return out, rec.calls


def _assert_handed(calls, name, view, layout):
    got = [x for n, x in calls if n == name]
    assert len(got) == 1, [n for n, _ in calls]
    x = got[0]
    if layout == "fallback":
        assert x.is_contiguous() and x.data_ptr() != view.data_ptr()
    else:
        assert x.data_ptr() == view.data_ptr(), f"{name} got a copy"
        assert x.stride() == view.stride()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


# ---------------------------------------------------------------------------
# routes: name -> (kinds, d, make(kind) -> (forest, rows), engine function,
# binding, env, oracle or None)
# ---------------------------------------------------------------------------


def _finite_rows(N, d, kind, seed):
    def make():
        X = _round(np.random.RandomState(seed)
                   .standard_normal((N, d)).astype(np.float32), kind)
        X.setflags(write=False)
        return X
    return _memo(("finite", N, d, kind, seed), make)


def _planted(N, d, kind, seed, value, cells):
    def make():
        X = np.array(_finite_rows(N, d, kind, seed))
        for r, c in cells:
            X[r, c] = value
        X.setflags(write=False)
        return X
    return _memo(("planted", N, d, kind, seed, str(value), cells), make)


def _std(d, N=N_ROWS, n=256, T=8):
    return lambda kind: (_forest(d, n, T, kind), _rows(N, d, kind, 5000 + d))


def _wide_std(kind):
    d = 4095

    def make():  # one forest for every row dtype: the splits are f32
        rs = np.random.RandomState(72)
        X = rs.normal(size=(2000, d)).astype(np.float32)
        bag = cpu_engine.sample_bags(2000, 3, 256, seed=21, bootstrap=False)
        fs = cpu_engine.feature_subsets(d, d, 3, seed=21)
        return cpu_engine.build_forest(X, bag, fs, 21, 256, d, d)
    forest = _memo(("wide-std",), make)
    assert not gpu_engine._packed_fits(forest, d)
    return forest, _finite_rows(N_ROWS, d, kind, 73)


def _wide_eif(kind):
    d = 5

    def make():
        rs = np.random.RandomState(73)
        X = rs.standard_normal((25000, d)).astype(np.float32)
        bag = cpu_engine.sample_bags(25000, 2, 17000, seed=22,
                                     bootstrap=False)
        fs = cpu_engine.feature_subsets(d, d, 2, seed=22)
        return cpu_engine.build_extended_forest(X, bag, fs, 22, 17000, d, d,
                                                d - 1)
    forest = _memo(("wide-eif",), make)
    assert forest.feature.shape[1] > 32767
    return forest, _finite_rows(N_ROWS, d, kind, 74)


def _eif(d, ext, rows, n=256, T=8):
    return lambda kind: (_forest(d, n, T, kind, ext=ext), rows(kind))


def _path_oracle(forest, X):
    with np.errstate(all="ignore"):
        if hasattr(forest, "hyper_w"):
            return cpu_engine.path_lengths_extended(forest, X)
        return cpu_engine.path_lengths(forest, X)


def _explain_oracle(forest, X):
    with np.errstate(all="ignore"):
        if hasattr(forest, "hyper_w"):
            return cpu_engine.feature_contributions_extended(forest, X, False)
        return cpu_engine.feature_contributions(forest, X, False)


_SCORE, _SCORE_EIF = "score_forest", "score_extended_forest"
_EXPLAIN, _EXPLAIN_EIF = "explain_forest", "explain_extended_forest"


def _dense_binding(kind):
    return ("score_extended_dense_v3" if kind == "bf16"
            else "score_extended_dense_v2")


# engine function, binding (a name or kind -> name), env, oracle
ROUTES = {
    # standard walk, rows staged in LDS (vector staging reachable at d = 32)
    "v4-d32": (KINDS, 32, _std(32), _SCORE, _SCORE, {}, _path_oracle),
    "v4-d33": (KINDS, 33, _std(33), _SCORE, _SCORE, {}, _path_oracle),
    # standard walk reading X inside the walk
    "v4-global-d32": (KINDS, 32, _std(32), _SCORE, _SCORE,
                      {"IFA_SCORE_FORCE_GLOBAL": "1"}, _path_oracle),
    "v4-global-d300": (["f32"], 300, _std(300), _SCORE, _SCORE, {},
                       _path_oracle),
    "wide-std": (KINDS, 4095, _wide_std, _SCORE, "score_forest_wide", {},
                 _path_oracle),
    # extended forests
    "eif0-on-v4": (KINDS, 5, _eif(5, 0, lambda k: _rows(N_ROWS, 5, k, 45,
                                                        nan=False),
                            n=64, T=9),
                   _SCORE_EIF, _SCORE, {}, _path_oracle),
    "sparse-v2": (KINDS, 8, _eif(8, 2, lambda k: _rows(N_ROWS, 8, k, 46)),
                  _SCORE_EIF, "score_extended_sparse_v2", {}, _path_oracle),
    "densified": (KINDS, 16,
                  _eif(16, 5, lambda k: _finite_rows(N_ROWS, 16, k, 47)),
                  _SCORE_EIF, _dense_binding, {}, None),
    "dense-nonfinite": (KINDS, 32,
                        _eif(32, 31, lambda k: _planted(
                            N_ROWS, 32, k, 48, np.inf, ((5, 3), (600, 31)))),
                        _SCORE_EIF, _dense_binding, {}, None),
    "old-dense": (["f32"], 68,
                  _eif(68, 67, lambda k: _finite_rows(N_ROWS, 68, k, 49)),
                  _SCORE_EIF, _SCORE_EIF, {}, None),
    "general": (KINDS, 16,
                _eif(16, 5, lambda k: _planted(N_ROWS, 16, k, 50, np.nan,
                                               ((300, 7),))),
                _SCORE_EIF, _SCORE_EIF, {}, _path_oracle),
    "wide-eif": (KINDS, 5, _wide_eif, _SCORE_EIF, "score_extended_wide", {},
                 _path_oracle),
    # attribution: accumulators and rows in LDS / global accumulators /
    # everything global
    "explain-1": (KINDS, 8, _std(8), _EXPLAIN, _EXPLAIN, {},
                  _explain_oracle),
    "explain-2": (KINDS, 8, _std(8), _EXPLAIN, _EXPLAIN,
                  {"IFA_EXPLAIN_FORCE_GLOBAL_ACC": "1"}, _explain_oracle),
    "explain-3": (["bf16"], 300, _std(300), _EXPLAIN, _EXPLAIN, {},
                  _explain_oracle),
    "explain-eif": (KINDS, 8, _eif(8, 2, lambda k: _rows(N_ROWS, 8, k, 46)),
                    _EXPLAIN_EIF, _EXPLAIN_EIF, {}, _explain_oracle),
}


def _route_cases():
    for route, spec in ROUTES.items():
        for kind in spec[0]:
            for layout in _layouts_for(spec[1]):
                yield pytest.param(route, kind, layout,
                                   id=f"{route}-{kind}-{layout}")


def _run_route(dev, monkeypatch, route, kind, layout):
    _, d, make, fn_name, binding, env, oracle = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if callable(binding):
        binding = binding(kind)
    forest, X = make(kind)
    assert X.shape[1] == d
    fn = getattr(gpu_engine, fn_name)
    shell = _memo(("shell", route, kind), lambda: Shell(forest))
    packed = _to_dev(X, kind, dev)
    view = _view(packed, layout)
    want = fn(shell, packed, finalize=False)
    got, calls = _recorded(fn, shell, view, finalize=False)
    assert [n for n, _ in calls] == [binding], calls
    _assert_handed(calls, binding, view, layout)
    np.testing.assert_array_equal(_bits(got), _bits(want),
                                  err_msg=f"{route} {kind} {layout}")
    if oracle is not None:
        ref = _memo(("ref", route, kind), lambda: oracle(forest, X))
        _assert_bitwise(got.cpu().numpy().reshape(-1), ref.reshape(-1),
                        f"{route} {kind} {layout} vs the CPU oracle")


class TestRoutes:
    @pytest.mark.parametrize("route,kind,layout", list(_route_cases()))
    def test_view_equals_packed(self, dev, monkeypatch, route, kind, layout):
        _run_route(dev, monkeypatch, route, kind, layout)


# ---------------------------------------------------------------------------
# row counts
# ---------------------------------------------------------------------------


class TestRowCounts:
    @pytest.mark.parametrize("kind", KINDS)
    @pytest.mark.parametrize("layout", ["pitched", "pitched16", "rowstep",
                                        "feature"])
    @pytest.mark.parametrize("route", ["v4", "sparse-v2"])
    def test_single_row(self, dev, route, layout, kind):
        """N = 1: torch's stride for the row dimension means nothing, the
        column stride still does."""
        d = 8
        if route == "v4":
            forest, fn, binding = (_forest(d, 256, 8, kind),
                                   gpu_engine.score_forest, _SCORE)
        else:
            forest, fn, binding = (_forest(d, 256, 8, kind, ext=2),
                                   gpu_engine.score_extended_forest,
                                   "score_extended_sparse_v2")
        X = _rows(N_ROWS, d, kind, 46)[300:301]
        shell = Shell(forest)
        packed = _to_dev(X, kind, dev)
        view = _view(packed, layout)
        got, calls = _recorded(fn, shell, view, finalize=False)
        assert [n for n, _ in calls] == [binding]
        _assert_handed(calls, binding, view, layout)
        np.testing.assert_array_equal(
            _bits(got), _bits(fn(shell, packed, finalize=False)))
        _assert_bitwise(got.cpu().numpy(), _path_oracle(forest, X),
                        f"N=1 {route} {kind} {layout}")

    @pytest.mark.parametrize("layout", ["pitched", "rowstep", "feature"])
    def test_grid_stride(self, dev, layout):
        """More than 8192 blocks of 512 rows: block 0 stages a second tile
        in its grid-stride loop (a tail), through 64-bit row offsets."""
        d, kind = 3, "bf16"
        forest = _forest(d, 8, 8, kind)
        N = MAX_BLOCKS * 512 + 513
        X = _rows(N, d, kind, 78)
        shell = _memo(("shell", "grid", kind), lambda: Shell(forest))
        view = _view(_to_dev(X, kind, dev), layout)
        got, calls = _recorded(gpu_engine.score_forest, shell, view,
                               finalize=False)
        _assert_handed(calls, _SCORE, view, layout)
        ref = _memo(("ref", "grid"), lambda: _path_oracle(forest, X))
        _assert_bitwise(got.cpu().numpy(), ref, f"grid-stride {layout}")


# ---------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------


class TestFit:
    @pytest.mark.parametrize("kind", KINDS)
    @pytest.mark.parametrize("layout", LAYOUTS)
    @pytest.mark.parametrize("est", [IsolationForest,
                                     ExtendedIsolationForest])
    def test_forest_equals_fit_on_packed(self, dev, est, layout, kind):
        """bag_gather reads the view; with a contamination the fit also
        scores the training rows, in place too."""
        d = 8
        packed = _to_dev(_finite_rows(N_ROWS, d, kind, 60), kind, dev)
        view = _view(packed, layout)
        kw = dict(numEstimators=8, maxSamples=256.0, randomSeed=11,
                  contamination=0.05)
        want = _memo(("fit", est.__name__, kind),
                     lambda: est(**kw).fit(packed))
        got, calls = _recorded(est(**kw).fit, view)
        _assert_handed(calls, "bag_gather", view, layout)
        scored = [n for n, _ in calls if n.startswith("score_")]
        assert len(scored) == 1, calls
        _assert_handed(calls, scored[0], view, layout)
        fields = ["feature", "value", "right", "num_instances", "node_count"]
        if est is ExtendedIsolationForest:
            fields += ["hyper_idx", "hyper_w", "offset64"]
        for f in fields:
            a, b = getattr(got.forest, f), getattr(want.forest, f)
            assert a.dtype == b.dtype and a.shape == b.shape, f
            assert a.tobytes() == b.tobytes(), f"{f} differs ({layout})"
        assert got.outlier_score_threshold == want.outlier_score_threshold


# ---------------------------------------------------------------------------
# the binding's own contract
# ---------------------------------------------------------------------------


class TestBinding:
    def _pack(self, dev, kind="f32", d=8):
        forest = _forest(d, 256, 8, kind)
        shell = _memo(("shell", "binding", kind), lambda: Shell(forest))
        aos, ncount, extra = gpu_engine._device_forest(
            shell, dev, v4_key=(d, kind))
        c = float(gpu_engine.avg_path_length(forest.num_samples))
        X = _to_dev(_rows(N_ROWS, d, kind, 46), kind, dev)

        def call(x):
            from isolation_forest_amd.ops import load_extension

            return load_extension().score_forest(
                x, aos, ncount, forest.num_trees, extra["height"], c, False)
        return X, call

    def test_rejects_other_strides_naming_them(self, dev):
        X, call = self._pack(dev)
        view = _view(X, "fallback")
        with pytest.raises(RuntimeError) as e:
            call(view)
        s0, s1 = view.stride()
        assert f"({s0}, {s1})" in str(e.value)
        assert "contiguous" not in str(e.value)

    def test_rejects_expanded_and_overlapping_rows(self, dev):
        X, call = self._pack(dev)
        with pytest.raises(RuntimeError, match=r"\(0, 1\)"):
            call(X[:1].expand(N_ROWS, 8))
        flat = X.reshape(-1)
        with pytest.raises(RuntimeError, match=r"\(7, 1\)"):
            call(flat.as_strided((100, 8), (7, 1)))

    @pytest.mark.parametrize("layout", IN_PLACE)
    def test_accepts_in_place_layouts(self, dev, layout):
        X, call = self._pack(dev)
        np.testing.assert_array_equal(_bits(call(_view(X, layout))),
                                      _bits(call(X)))


# ---------------------------------------------------------------------------
# no hidden copy, by allocation
# ---------------------------------------------------------------------------


class TestNoHiddenCopy:
    def test_score_and_fit_allocate_no_second_matrix(self, dev):
        N, d = 2 ** 20, 32
        g = torch.Generator(device=dev).manual_seed(5)
        buf = torch.randn(d, N, generator=g, device=dev)
        view = buf.T  # feature-major [N, d], 128 MiB
        view_bytes = view.numel() * view.element_size()
        assert gpu_engine._row_layout(view) == "feature"
        model = IsolationForest(numEstimators=16, maxSamples=256.0,
                                randomSeed=3, contamination=0.0
                                ).fit(view[:4096])
        model.score(view[:1000])  # builds the packs

        def peak_of(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
            print(f"peak extra allocation {peak / 2 ** 20:.2f} MiB "
                  f"(view {view_bytes / 2 ** 20:.0f} MiB)")
            return out, peak

        scores, peak = peak_of(lambda: model.score(view))
        assert scores.shape == (N,)
        assert peak < view_bytes // 4, peak
        est = IsolationForest(numEstimators=16, maxSamples=256.0,
                              randomSeed=3, contamination=0.0)
        fitted, peak = peak_of(lambda: est.fit(view))
        assert fitted.forest.num_trees == 16
        assert peak < view_bytes // 4, peak


# ---------------------------------------------------------------------------
# 64-bit offsets
# ---------------------------------------------------------------------------


class Test64BitOffsets:
    def test_column_stride_past_2_31(self, dev):
        """Feature-major with a column stride of 2^31 + 8 elements at
        storage offset 2^31: a 32-bit column offset, signed or unsigned,
        puts column 1 or 2 on an address that is still inside the
        allocation, and those places hold NaN."""
        if torch.cuda.mem_get_info()[0] < 32 * 2 ** 30:
            pytest.skip("needs 32 GiB of free device memory")
        N, d, kind = 1000, 3, "bf16"
        cs, off = 2 ** 31 + 8, 2 ** 31
        store = torch.empty(3 * 2 ** 31 + 8192, dtype=torch.bfloat16,
                            device=dev)
        for p in (0, 8, 16, 2 ** 31 + 16, 2 ** 32):
            store[p:p + 2048] = float("nan")
        view = store.as_strided((N, d), (1, cs), off)
        X = _rows(N, d, kind, 79, nan=False)
        packed = _to_dev(X, kind, dev)
        view.copy_(packed)
        assert torch.equal(view.contiguous().view(torch.int16),
                           packed.view(torch.int16))
        assert gpu_engine._row_layout(view) == "feature"

        forest = _forest(d, 8, 8, kind)
        shell = Shell(forest)
        got, calls = _recorded(gpu_engine.score_forest, shell, view,
                               finalize=False)
        _assert_handed(calls, _SCORE, view, "feature")
        np.testing.assert_array_equal(
            _bits(got),
            _bits(gpu_engine.score_forest(shell, packed, finalize=False)))
        _assert_bitwise(got.cpu().numpy(), _path_oracle(forest, X),
                        "64-bit column offsets")

        kw = dict(numEstimators=8, maxSamples=256.0, randomSeed=11,
                  contamination=0.0)
        a, calls = _recorded(IsolationForest(**kw).fit, view)
        _assert_handed(calls, "bag_gather", view, "feature")
        b = IsolationForest(**kw).fit(packed)
        for f in ("feature", "value", "right", "num_instances"):
            assert (getattr(a.forest, f).tobytes()
                    == getattr(b.forest, f).tobytes()), f
