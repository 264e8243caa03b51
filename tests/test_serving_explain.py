"""POST /v1/explain (FastAPI TestClient, CPU): the response carries the
model's feature contributions, its expected path length and the scores;
request validation is /v1/score's."""

import numpy as np
import pytest
import torch

pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

from isolation_forest_amd import (  # noqa: E402
    ExtendedIsolationForest,
    IsolationForest,
)
from isolation_forest_amd.serving import create_app  # noqa: E402


@pytest.fixture(scope="module", params=["standard", "extended"])
def served(request, tmp_path_factory, gaussian_data):
    X, _ = gaussian_data
    est = (IsolationForest(numEstimators=20, randomSeed=21)
           if request.param == "standard"
           else ExtendedIsolationForest(numEstimators=20, randomSeed=21))
    model = est.fit(X)
    path = str(tmp_path_factory.mktemp("explain") / request.param)
    model.save(path)
    return model, X, TestClient(create_app(path, device="cpu"))


def test_response_matches_model_call(served):
    model, X, client = served
    rows = X[:32]
    r = client.post("/v1/explain", json={"instances": rows.tolist()})
    assert r.status_code == 200
    body = r.json()
    assert set(body) == {"contributions", "expectedPathLength", "scores"}
    xt = torch.from_numpy(rows)
    want = model.feature_contributions(xt).numpy()
    got = np.asarray(body["contributions"], dtype=np.float32)
    # JSON carries the float32 values widened to double: exact round trip
    np.testing.assert_array_equal(got, want)
    assert body["expectedPathLength"] == model.expected_path_length
    np.testing.assert_array_equal(
        np.asarray(body["scores"], dtype=np.float32),
        model.score(xt).numpy())


def test_bad_widths_return_400(served):
    _, X, client = served
    r = client.post("/v1/explain", json={"instances": [[1.0, 2.0]]})
    assert r.status_code == 400
    assert "features" in r.json()["detail"]
    r = client.post("/v1/explain", json={"instances": [[1, 2, 3], [1, 2]]})
    assert r.status_code == 400


def test_empty_batch(served):
    model, _, client = served
    r = client.post("/v1/explain", json={"instances": []})
    assert r.status_code == 200
    assert r.json() == {"contributions": [], "scores": [],
                        "expectedPathLength": model.expected_path_length}
