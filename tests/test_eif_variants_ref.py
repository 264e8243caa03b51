"""The case table of tests/test_eif_variants_gpu.py, checked without a GPU:
every case reaches the kernel variant it was chosen for, the order-exact
references of tests/eif_order_ref.py are right, and the planted knife-edge
rows really separate the summation orders (otherwise a bitwise GPU test
against them would prove no more than oracle parity).

Unreachable instances of score_extended_forest_kernel<XT, ROWS_LDS,
HYPER_LDS, NODES_LDS>: (T,T,F) and (F,T,F). Nodes leave LDS above 15360 per
tree (8 B each against 120 KiB), while hyperplanes in LDS need
max_nodes * nnz * 8 <= 96 KiB, i.e. at most 12288 nodes even at nnz = 1: a
forest whose nodes are global always has global hyperplanes.
"""

from fractions import Fraction

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from tests import eif_order_ref as R

N_SCORE = 3001  # coprime with every tile size
# Share of the rows moved onto a hyperplane. At d = 5 the fused and the
# unfused 4-chain dot differ in a single rounding (chain 0 alone holds two
# terms), so fewer planted rows tell them apart there than at d >= 8; three
# quarters leave room above the 50 rows TestKnifeEdges asks for.
PLANT_FRAC = 0.75

_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------
# forests: ("trained", n, d, T, ext) | ("complete", height, nnz, d, T)
# ---------------------------------------------------------------------------


def forest_of(spec):
    def make():
        if spec[0] == "trained":
            return R.trained_extended_forest(*spec[1:])
        return R.complete_extended_forest(*spec[1:], seed=29)
    return memo(("forest", spec), make)


def _trained(n, d, T, nnz):
    return ("trained", n, d, T, nnz - 1)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------

T_, F_ = True, False

# id -> (forest spec, d, row kind, how the binding is reached, expected
# (rows_lds, hyper_lds, nodes_lds)). "router": gpu_engine's router must hand
# the call to the score_extended_forest binding by itself; "direct": the
# binding is called with the engine's pack (the router would pick sparse v2
# or a dense kernel for that shape).
GENERAL_CASES = {
    # rows boundary: 256 rows of d + 16/elem cells against 144 KiB
    "rows-f32-d132": (_trained(128, 132, 5, 3), 132, "f32", "router",
                      (T_, T_, T_)),
    "rows-f32-d133": (_trained(128, 133, 5, 3), 133, "f32", "router",
                      (F_, T_, T_)),
    "rows-bf16-d264": (_trained(128, 264, 5, 3), 264, "bf16", "router",
                       (T_, T_, T_)),
    "rows-bf16-d265": (_trained(128, 265, 5, 3), 265, "bf16", "router",
                       (F_, T_, T_)),
    "rows-f16-d264": (_trained(128, 264, 5, 3), 264, "f16", "router",
                      (T_, T_, T_)),
    "rows-f16-d265": (_trained(128, 265, 5, 3), 265, "f16", "router",
                      (F_, T_, T_)),
    # hyperplane boundary: 2047 nodes, 8 B per coordinate against 96 KiB
    "hyper-nnz5": (_trained(1024, 7, 3, 5), 7, "f32", "direct",
                   (T_, T_, T_)),
    "hyper-nnz6": (_trained(1024, 7, 3, 6), 7, "f32", "direct",
                   (T_, F_, T_)),
    "hyper-nnz6-bf16": (_trained(1024, 7, 3, 6), 7, "bf16", "direct",
                        (T_, F_, T_)),
    # rows and hyperplanes global, nodes staged
    "rowshyper-f32-d125": (_trained(1024, 125, 3, 6), 125, "f32", "direct",
                           (F_, F_, T_)),
    "rowshyper-bf16-d250": (_trained(1024, 250, 3, 6), 250, "bf16", "direct",
                            (F_, F_, T_)),
    "rowshyper-f16-d250": (_trained(1024, 250, 3, 6), 250, "f16", "direct",
                           (F_, F_, T_)),
    # node boundary: 8191 / 16383 slots of 8 B against 120 KiB
    "nodes-n4096": (_trained(4096, 7, 2, 3), 7, "f32", "router",
                    (T_, F_, T_)),
    "nodes-n4097": (_trained(4097, 7, 2, 3), 7, "f32", "router",
                    (T_, F_, F_)),
    "allglobal-n8192": (_trained(8192, 144, 2, 3), 144, "f32", "router",
                        (F_, F_, F_)),
    # every node slot live: ids up to 16382 are walked
    "highid-f32-d7": (("complete", 13, 3, 7, 2), 7, "f32", "router",
                      (T_, F_, F_)),
    "highid-f16-d7": (("complete", 13, 3, 7, 2), 7, "f16", "router",
                      (T_, F_, F_)),
    "highid-f32-d144": (("complete", 13, 3, 144, 2), 144, "f32", "router",
                        (F_, F_, F_)),
    "highid-bf16-d288": (("complete", 13, 3, 288, 2), 288, "bf16", "router",
                         (F_, F_, F_)),
    "highid-f16-d288": (("complete", 13, 3, 288, 2), 288, "f16", "router",
                        (F_, F_, F_)),
}

# (d, kind) -> expected (rows_lds, wlds) of the old dense kernel; nnz = d,
# d % 4 = 0, n = 128 (255 node slots), all reached through the router
OLD_DENSE_T = 5
OLD_DENSE_CASES = {
    (72, "f32"): (T_, T_),
    (72, "f16"): (T_, T_),
    (76, "f32"): (T_, F_),
    (144, "f32"): (T_, F_),
    (148, "f32"): (F_, F_),
    (96, "f16"): (T_, T_),
    (100, "f16"): (T_, F_),
    (132, "bf16"): (T_, F_),
    (300, "bf16"): (F_, F_),
    (300, "f16"): (F_, F_),
}

# (d, D, kind): dense v2 with nnz = d; bf16 rows reach it under
# IFA_EIF_DENSE_V2=1
DENSE_V2_T = 8
DENSE_V2_CASES = [
    (5, 8, "f32"), (8, 8, "f32"), (13, 16, "f32"), (31, 32, "f32"),
    (40, 64, "f32"), (64, 64, "f32"),
    (13, 16, "f16"), (40, 64, "f16"), (13, 16, "bf16"), (40, 64, "bf16"),
]
# densified: 6 <= nnz < d (d, ext, D)
DENSIFIED_V2 = (12, 7, 16)


def old_dense_spec(d):
    return _trained(128, d, OLD_DENSE_T, d)


def dense_v2_spec(d):
    return _trained(128, d, DENSE_V2_T, d)


def densified_spec():
    d, ext, _ = DENSIFIED_V2
    return ("trained", 128, d, DENSE_V2_T, ext)


def dense_id(case):
    return "-".join(str(c) for c in case)


# ---------------------------------------------------------------------------
# rows (f32 arrays exact in the row dtype, memoised and read-only)
# ---------------------------------------------------------------------------


def gauss_rows(d, kind, zero_row=False):
    def make():
        X = R.round_rows(np.random.RandomState(3000 + d)
                         .normal(size=(N_SCORE, d)).astype(np.float32), kind)
        if zero_row:
            X[0] = 0.0  # goes right at every offset-0 node
        return _frozen(X)
    return memo(("gauss", d, kind, zero_row), make)


def planted_rows(forest_spec, d, kind):
    def make():
        X = gauss_rows(d, kind)
        return _frozen(R.plant_knife_edges(
            forest_of(forest_spec), X, np.random.RandomState(5), PLANT_FRAC,
            kind))
    return memo(("planted", forest_spec, d, kind), make)


def reference(forest_spec, X, mode, D=None):
    """Memoised path sums; mode "oracle" is cpu_engine's own walk."""
    def make():
        f = forest_of(forest_spec)
        with np.errstate(all="ignore"):
            if mode == "oracle":
                return X, cpu_engine.path_lengths_extended(f, X)
            return X, R.walk_chain4(f, X, mode, D)
    # keyed by identity: the rows are memoised and kept alive in the value
    return memo(("ref", forest_spec, id(X), mode, D), make)[1]


def _differ(a, b):
    return int((a.view(np.int32) != b.view(np.int32)).sum())


# ---------------------------------------------------------------------------
# 1. fma32 against exact rational arithmetic
# ---------------------------------------------------------------------------


def _round_fraction_f32(fr):
    """Nearest-even f32 of a Fraction, denormals kept, overflow to inf."""
    if fr == 0:
        return np.float32(0.0)
    sign = -1 if fr < 0 else 1
    fr = abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1  # 2^e <= fr < 2^(e+1)
    q = max(e, -126) - 23  # weight of the last kept bit
    scaled = fr / Fraction(2) ** q
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    with np.errstate(over="ignore"):
        return np.float32(sign * float(m) * 2.0 ** q)  # exact below 2^128


def _exact_fma(a, b, c):
    return _round_fraction_f32(
        Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _fma_triples(n=17000):
    rs = np.random.RandomState(0)
    parts = []

    def wide():  # Gaussian mantissas over 40 binades
        return (rs.normal(size=n) * 2.0 ** rs.randint(-20, 20, size=n)
                ).astype(np.float32)
    parts.append((wide(), wide(), wide()))
    # near-total cancellation: c ~ -a * b, and c one f32 step off -a * b
    a, b = (rs.normal(size=n).astype(np.float32) for _ in range(2))
    p = a.astype(np.float64) * b
    parts.append((a, b, (-p * (1 + rs.normal(size=n) * 1e-7))
                  .astype(np.float32)))
    parts.append((a, b, np.nextafter(
        (-p).astype(np.float32),
        rs.choice([-np.inf, np.inf], size=n).astype(np.float32))))
    # denormal results: tiny products next to tiny or zero addends
    a = (rs.normal(size=n) * 2.0 ** -70).astype(np.float32)
    b = (rs.normal(size=n) * 2.0 ** -65).astype(np.float32)
    parts.append((a, b, (rs.normal(size=n) * 2.0 ** -140)
                  .astype(np.float32)))
    parts.append((a, b, np.zeros(n, dtype=np.float32)))
    # double-rounding ties. c = +-M * 2^30 with a 24-bit M, so c's f32 step
    # is 2^30 and |c| >= 2^53, where the f64 step is 2. The product
    # +-2^14 (1 + e) * 2^15 (1 - e) = +-(2^29 - 2^(29-2k)), e = 2^-k with
    # 15 <= k <= 23, is half an f32 step of c less a tail below half an f64
    # step: the f64 sum lands exactly ON the f32 midpoint and only TwoSum's
    # error knows the side. Half of these resolve against ties-to-even.
    M = rs.randint(2 ** 23, 2 ** 24, size=n).astype(np.float64)
    c = (M * rs.choice([-1.0, 1.0], size=n) * 2.0 ** 30).astype(np.float32)
    e = 2.0 ** -rs.randint(15, 24, size=n)
    a = (rs.choice([-1.0, 1.0], size=n) * 2.0 ** 14 * (1 + e)).astype(
        np.float32)
    b = (2.0 ** 15 * (1 - e)).astype(np.float32)
    parts.append((a, b, c))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


class TestFma32:
    def test_against_exact_rationals(self):
        """>= 10^5 triples: random, cancelling, denormal results, and
        constructed double-rounding ties; the tie correction must fire."""
        a, b, c = _fma_triples()
        assert len(a) >= 100000
        stats = {}
        got = R.fma32(a, b, c, stats)
        want = np.array([_exact_fma(*t) for t in zip(a, b, c)],
                        dtype=np.float32)
        bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
        assert len(bad) == 0, (len(bad), a[bad[:4]], b[bad[:4]], c[bad[:4]],
                               got[bad[:4]], want[bad[:4]])
        assert stats["ties"] >= 1000, stats
        # the plain f64 route (no correction) misses exactly those
        with np.errstate(all="ignore"):
            naive = (a.astype(np.float64) * b + c).astype(np.float32)
        assert _differ(naive, want) == stats["ties"]
        den = (want != 0) & (np.abs(want) < np.float32(1.1754944e-38))
        assert den.sum() >= 1000, int(den.sum())

    def test_nonfinite_follow_ieee(self):
        inf, nan = np.float32(np.inf), np.float32(np.nan)
        a = np.array([inf, inf, 0.0, 3e38, 3e38, nan, -inf], np.float32)
        b = np.array([1.0, 0.0, 5.0, 2.0, 2.0, 1.0, 1.0], np.float32)
        c = np.array([1.0, 1.0, -0.0, 0.0, -inf, 1.0, inf], np.float32)
        got = R.fma32(a, b, c)
        assert got[0] == inf and np.isnan(got[1]) and got[2] == 0
        assert got[3] == inf and got[4] == -inf and np.isnan(got[5])
        assert np.isnan(got[6])


# ---------------------------------------------------------------------------
# 2. the walker itself
# ---------------------------------------------------------------------------


class TestWalker:
    @pytest.mark.parametrize("spec,d", [
        (_trained(128, 16, 8, 16), 16), (_trained(128, 12, 8, 8), 12),
        (_trained(1024, 7, 3, 5), 7), (("complete", 13, 3, 7, 2), 7)],
        ids=["dense-d16", "nnz8-d12", "nnz5-n1024", "complete"])
    def test_strict_mode_is_the_oracle(self, spec, d):
        f = forest_of(spec)
        for X in (gauss_rows(d, "f32"), planted_rows(spec, d, "f32")):
            got = R.walk_chain4(f, X, "strict")
            assert _differ(got, reference(spec, X, "oracle")) == 0

    def test_padding_to_D_changes_nothing(self):
        """Zero weight times zero cell adds +0 to a chain."""
        spec = _trained(128, 13, 8, 13)
        f, X = forest_of(spec), planted_rows(spec, 13, "f32")
        for mode in ("muladd", "fma"):
            assert _differ(R.walk_chain4(f, X, mode),
                           R.walk_chain4(f, X, mode, 16)) == 0

    def test_complete_forest_walks_every_id_range(self):
        spec = ("complete", 13, 3, 7, 2)
        f = forest_of(spec)
        assert f.feature.shape == (2, 16383)
        assert (f.node_count == 16383).all() and (f.feature >= -1).all()
        leaves = f.feature[0] == -1
        assert leaves.sum() == 8192
        assert len(np.unique(f.value[0][leaves])) == 8192
        trace = {}
        ps = R.walk_chain4(f, gauss_rows(7, "f32", zero_row=True), "strict",
                           trace=trace)
        assert trace["max_node"] == 16382
        # the rows spread over the leaves
        assert len(np.unique(ps)) > N_SCORE // 2


# ---------------------------------------------------------------------------
# 3. knife-edge rows separate the orders
# ---------------------------------------------------------------------------


def knife_cases():
    """(forest spec, d, D, row kind, the kernel's mode) of every dense case:
    its planted rows must separate the summation orders."""
    out = []
    for (d, kind) in OLD_DENSE_CASES:
        out.append(pytest.param(old_dense_spec(d), d, d, kind, "muladd",
                                id=f"old-dense-{d}-{kind}"))
    for (d, D, kind) in DENSE_V2_CASES:
        out.append(pytest.param(dense_v2_spec(d), d, D, kind, "fma",
                                id=f"dense-v2-{d}-{kind}"))
    d, _, D = DENSIFIED_V2
    out.append(pytest.param(densified_spec(), d, D, "f32", "fma",
                            id="densified-v2"))
    return out


class TestKnifeEdges:
    @pytest.mark.parametrize("spec,d,D,kind,mode", knife_cases())
    def test_planted_rows_separate_the_orders(self, spec, d, D, kind, mode):
        Xg, Xp = gauss_rows(d, kind), planted_rows(spec, d, kind)
        oracle = reference(spec, Xp, "oracle")
        mul = reference(spec, Xp, "muladd", D)
        fma = reference(spec, Xp, "fma", D)
        own = mul if mode == "muladd" else fma
        on_gauss = _differ(reference(spec, Xg, mode, D),
                           reference(spec, Xg, "oracle"))
        print(f"[knife] d={d} D={D} {kind}: {mode} vs oracle "
              f"{_differ(own, oracle)}, fma vs muladd {_differ(fma, mul)}; "
              f"on Gaussian rows {on_gauss}")
        assert _differ(own, oracle) >= 100
        assert _differ(fma, mul) >= 50


# ---------------------------------------------------------------------------
# 4. every case reaches its variant
# ---------------------------------------------------------------------------


def _mn(spec):
    if spec[0] == "trained":
        return R.max_nodes_for(spec[1])
    return 2 ** (spec[1] + 1) - 1


class TestVariants:
    @pytest.mark.parametrize("case", list(GENERAL_CASES))
    def test_general_case(self, case):
        spec, d, kind, via, want = GENERAL_CASES[case]
        f = forest_of(spec)
        mn, nnz, elem = f.feature.shape[1], f.nnz, R.ELEM[kind]
        assert mn == _mn(spec) and f.total_num_features == d
        assert not R.takes_old_dense(d, mn, nnz)
        assert R.general_variant(d, mn, nnz, elem) == want
        if via == "router":
            assert nnz <= 5 and R.sparse_v2_declines(d, mn, nnz, elem)
        # the walk is deep enough to use what is staged
        assert int(f.node_count.max()) > 50

    def test_general_boundaries_pair_up(self):
        """Each boundary is crossed by one step of one quantity."""
        g = {k: v[4] for k, v in GENERAL_CASES.items()}
        for a, b, axis in [("rows-f32-d132", "rows-f32-d133", 0),
                           ("rows-bf16-d264", "rows-bf16-d265", 0),
                           ("rows-f16-d264", "rows-f16-d265", 0),
                           ("hyper-nnz5", "hyper-nnz6", 1),
                           ("nodes-n4096", "nodes-n4097", 2)]:
            flipped = [i for i in range(3) if g[a][i] != g[b][i]]
            assert flipped == [axis] and g[a][axis] and not g[b][axis], (a, b)
        reached = set(g.values())
        assert reached == {(T_, T_, T_), (F_, T_, T_), (T_, F_, T_),
                           (F_, F_, T_), (T_, F_, F_), (F_, F_, F_)}
        for variant in reached:  # each with f32 and with 16-bit rows
            kinds = {v[2] for v in GENERAL_CASES.values() if v[4] == variant}
            assert "f32" in kinds and kinds & {"bf16", "f16"}, variant

    def test_unreachable_instances(self):
        """(T,T,F) and (F,T,F): global nodes imply global hyperplanes."""
        for mn in (15361, 16383, 32767):
            assert mn * 8 > 120 * 1024
            for elem in (2, 4):
                for d in (1, 7, 4095):
                    v = R.general_variant(d, mn, 1, elem)
                    assert v[1:] == (F_, F_), (mn, d, v)

    @pytest.mark.parametrize("case", list(OLD_DENSE_CASES), ids=dense_id)
    def test_old_dense_case(self, case):
        d, kind = case
        f = forest_of(old_dense_spec(d))
        mn = f.feature.shape[1]
        assert mn == 255 and f.nnz == d
        assert R.takes_old_dense(d, mn, f.nnz)
        assert R.old_dense_variant(d, mn, R.ELEM[kind]) == \
            OLD_DENSE_CASES[case]
        # the router passes it on: too wide for dense v2, and for dense v3
        # (bf16 rows only) past d = 128
        assert d > 64 and (kind != "bf16" or d > 128)

    def test_old_dense_boundaries_pair_up(self):
        o = OLD_DENSE_CASES
        assert o[(72, "f32")] == (T_, T_) and o[(76, "f32")] == (T_, F_)
        assert o[(144, "f32")] == (T_, F_) and o[(148, "f32")] == (F_, F_)
        assert o[(96, "f16")] == (T_, T_) and o[(100, "f16")] == (T_, F_)
        assert set(o.values()) == {(T_, T_), (T_, F_), (F_, F_)}
        # (F, T) cannot be: weights are staged only if the rows fit as well
        for d in range(4, 4096, 4):
            for elem in (2, 4):
                assert R.old_dense_variant(d, 255, elem) != (F_, T_)

    @pytest.mark.parametrize("case", DENSE_V2_CASES, ids=dense_id)
    def test_dense_v2_case(self, case):
        d, D, kind = case
        f = forest_of(dense_v2_spec(d))
        assert f.nnz == d and D == next(x for x in (8, 16, 32, 64) if d <= x)
        mn = f.feature.shape[1]
        assert mn * 12 + 16 + mn * (D // 4 + 1) * 16 <= 160 * 1024

    def test_densified_case(self):
        d, ext, D = DENSIFIED_V2
        f = forest_of(densified_spec())
        assert 6 <= f.nnz < d and f.nnz == ext + 1 and D == 16
