"""No GPU: where gpu_engine.large_shap_route sends TreeSHAP for forests past
the 15-bit node ids, and the [33, 32] Shapley weight table the deep kernel
stages (docs/DESIGN.md §9)."""

import dataclasses
import math
import types

import numpy as np
import pytest
import torch

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine
from tests.test_score_deep_gpu import Shell
from tests.test_shap_deep_gpu import MN, chain


def narrow(forest, width=100):
    """The same trees in arrays that fit the packed formats."""
    cut = {f.name: getattr(forest, f.name)[:, :width].copy()
           for f in dataclasses.fields(forest)
           if getattr(getattr(forest, f.name), "ndim", 0) == 2}
    return dataclasses.replace(forest, **cut)


@pytest.mark.parametrize("features,d,env,width,want", [
    (range(32), 35, None, MN, "deep"),
    (range(32), 4094, None, MN, "deep"),
    (range(33), 36, None, MN, "cpu"),    # max_m = 33
    ([4095], 4096, None, MN, "cpu"),     # a feature id past 12 bits
    ([3], 4095, None, MN, "cpu"),        # d is the 12-bit leaf sentinel
    (range(32), 35, "0", MN, "cpu"),     # IFA_SHAP_DEEP=0
    (range(32), 35, None, 100, "cpu"),   # node arrays that fit the packed ids
])
def test_route(monkeypatch, features, d, env, width, want):
    features = list(features)
    forest = chain(features, np.zeros(len(features), dtype=np.float32))
    if width != MN:
        forest = narrow(forest, width)
    assert cpu_engine.shap_tables(forest)["max_m"] == len(features)
    if env is not None:
        monkeypatch.setenv("IFA_SHAP_DEEP", env)
    for dtype in (torch.float32, torch.bfloat16, "f16"):
        assert gpu_engine.large_shap_route(forest, d, dtype) == want


def test_route_caps_the_nodes_of_a_tree():
    forest = chain([0, 1], np.zeros(2, dtype=np.float32))
    forest.node_count[0] = gpu_engine.DEEP_MAX_NODES + 1
    assert gpu_engine.large_shap_route(forest, 5, "f32") == "cpu"
    assert cpu_engine.SHAP_DEEP_MAX_PATH_FEATURES == 32
    assert cpu_engine.SHAP_MAX_PATH_FEATURES == 16


def test_a_packed_size_forest_never_reaches_the_route(monkeypatch):
    forest = narrow(chain([0, 1, 2], np.float32([-0.5, 0.0, 0.5])))
    assert gpu_engine._packed_fits(forest, 3)

    def no_route(*args):
        raise AssertionError("large_shap_route consulted")

    monkeypatch.setattr(gpu_engine, "large_shap_route", no_route)
    monkeypatch.setattr(
        gpu_engine, "load_extension",
        lambda: types.SimpleNamespace(shap_forest=lambda *a: "packed kernel"))
    assert gpu_engine.shap_forest(Shell(forest), torch.zeros((4, 3)),
                                  True) == "packed kernel"


def test_weights_sum_to_one_against_the_binomials():
    # sum_k C(m-1, k) w[m][k] = 1 exactly. Each w is the correctly rounded
    # quotient of exact integers (one rounding, u = 2^-53), C(m-1, k) <
    # 2^53 is exact, the product rounds once more, and the m - 1 adds of
    # the positive terms round once each: (1 + u)^(m + 1) - 1 <=
    # gamma(m + 1) = (m + 1) u / (1 - (m + 1) u)  (Higham, Lemma 3.1).
    w = cpu_engine.shap_weights(cpu_engine.SHAP_DEEP_MAX_PATH_FEATURES)
    assert w.shape == (33, 32) and w.dtype == np.float64
    u = 2.0 ** -53
    for m in range(1, 33):
        total = 0.0
        for k in range(m):
            total += float(math.comb(m - 1, k)) * float(w[m, k])
        assert abs(total - 1.0) <= (m + 1) * u / (1 - (m + 1) * u), m
        assert not w[m, m:].any()
    assert not w[0].any()


def test_rows_up_to_16_are_the_default_table():
    small = cpu_engine.shap_weights()
    big = cpu_engine.shap_weights(32)
    assert small.shape == (17, 16)
    np.testing.assert_array_equal(big[:17, :16].view(np.int64),
                                  small.view(np.int64))
    assert not big[:17, 16:].any()
