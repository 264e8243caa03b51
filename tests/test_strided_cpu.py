"""Input layouts, the part that needs no GPU: the classifier that decides
which 2-D row views the GPU kernels consume in place
(ops/gpu_engine._row_layout / _rows_in_place), exercised on CPU tensors,
and a pin that the CPU engine's results do not depend on the view's layout.

Contract (docs/API.md "Input layouts"): with (rs, cs) = X.stride(),
pitched row-major is cs == 1 and rs >= d, feature-major is rs == 1 and
cs >= N; the stride of a size-1 dimension is ignored; a view that fits both
is row-major; everything else is copied once.
"""

import logging

import numpy as np
import pytest
import torch

from isolation_forest_amd import ExtendedIsolationForest, IsolationForest
from isolation_forest_amd.ops import gpu_engine

N, D = 37, 6


def _packed():
    return torch.arange(N * D, dtype=torch.float32).reshape(N, D)


def _views():
    """name -> (view, expected strides or None, expected class)."""
    a = np.arange(N * D, dtype=np.float32).reshape(N, D)
    wide = torch.zeros(N + 5, D + 11)
    tall = torch.zeros(2 * N, D)
    fm = torch.zeros(D + 2, N + 7)
    return {
        "packed": (_packed(), (D, 1), "row"),
        "pitched": (wide[2:2 + N, 3:3 + D], (D + 11, 1), "row"),
        "rowstep": (tall[::2], (2 * D, 1), "row"),
        "feature": (fm[1:1 + D, 4:4 + N].T, (1, N + 7), "feature"),
        "fortran": (torch.from_numpy(np.asfortranarray(a)), (1, N),
                    "feature"),
        "colstep": (torch.zeros(N, 2 * D)[:, ::2], (2 * D, 2), None),
        "expand": (torch.zeros(1, D).expand(N, D), (0, 1), None),
        "one-column": (torch.zeros(N, 1), None, "row"),
        "one-row": (torch.zeros(1, D), None, "row"),
        "one-row-T": (torch.zeros(D, 1).T, None, "row"),
    }


class TestClassifier:
    @pytest.mark.parametrize("name", list(_views()))
    def test_class(self, name):
        view, strides, want = _views()[name]
        if strides is not None:
            assert tuple(view.stride()) == strides
        assert gpu_engine._row_layout(view) == want

    def test_size_one_dimension_stride_is_ignored(self):
        # a [N, 1] column of a wider table (row stride 9) and a [1, d] row
        # of a feature-major buffer (column stride 50): the size-1
        # dimension's stride says nothing
        assert gpu_engine._row_layout(torch.zeros(N, 9)[:, 4:5]) == "row"
        assert gpu_engine._row_layout(torch.zeros(D, 50).T[7:8]) == "feature"
        assert gpu_engine._row_layout(torch.zeros(1, 1)) == "row"

    def test_overlapping_rows_are_not_in_place(self):
        base = torch.zeros(N * D)
        assert gpu_engine._row_layout(
            base.as_strided((N, D), (D - 1, 1))) is None
        assert gpu_engine._row_layout(
            base.as_strided((N, D), (1, N - 1))) is None

    @pytest.mark.parametrize("name", list(_views()))
    def test_rows_in_place(self, name, caplog):
        view, _, want = _views()[name]
        with caplog.at_level(logging.DEBUG, logger=gpu_engine.__name__):
            got = gpu_engine._rows_in_place(view)
        if want is None:
            assert got is not view and got.is_contiguous()
            assert torch.equal(got, view)
            assert str(tuple(view.stride())) in caplog.text
        else:
            assert got is view
            assert caplog.text == ""


# ---------------------------------------------------------------------------
# the CPU path did not move: every view scores, fits and explains exactly
# like its packed copy
# ---------------------------------------------------------------------------


def _data_views():
    rs = np.random.RandomState(3)
    a = rs.standard_normal((400, 5)).astype(np.float32)
    X = torch.from_numpy(a)
    wide = torch.full((405, 16), float("nan"))
    wide[2:402, 3:8] = X
    tall = torch.full((800, 5), float("nan"))
    tall[::2] = X
    fm = torch.full((7, 407), float("nan"))
    fm[1:6, 4:404] = X.T
    two = torch.full((400, 10), float("nan"))
    two[:, ::2] = X
    return {
        "packed": X,
        "pitched": wide[2:402, 3:8],
        "rowstep": tall[::2],
        "feature": fm[1:6, 4:404].T,
        "fortran": torch.from_numpy(np.asfortranarray(a)),
        "colstep": two[:, ::2],
    }


def _bits(t):
    return t.contiguous().numpy().view(np.int32)


@pytest.mark.parametrize("est", [IsolationForest, ExtendedIsolationForest])
@pytest.mark.parametrize("name", list(_data_views()))
def test_cpu_results_do_not_depend_on_layout(est, name):
    view = _data_views()[name]
    packed = view.contiguous()
    assert torch.equal(view, packed)
    kw = dict(numEstimators=8, maxSamples=64.0, randomSeed=5,
              contamination=0.05)
    m_view, m_packed = est(**kw).fit(view), est(**kw).fit(packed)
    for field in ("feature", "value", "right", "num_instances"):
        np.testing.assert_array_equal(getattr(m_view.forest, field),
                                      getattr(m_packed.forest, field))
    assert m_view.outlier_score_threshold == m_packed.outlier_score_threshold
    np.testing.assert_array_equal(_bits(m_packed.score(view)),
                                  _bits(m_packed.score(packed)))
    np.testing.assert_array_equal(
        _bits(m_packed.feature_contributions(view)),
        _bits(m_packed.feature_contributions(packed)))
