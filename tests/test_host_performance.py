"""CPU-side tests of the deterministic evaluation harness (pulpo_amd.evaluation): the keys of the reference golden, the aggregation of
PerformanceTable (evaluate.py:1476-1488), the landmark metrics, argument errors, and the host-side size queries of the two new entry points."""
import warnings

import numpy as np
import pytest
import torch

METRICS = ["RMSE", "JDetStd", "JDetLeq0", "Dice", "LM_MAE", "LM_Euclid"]


def test_performance_golden_keys_and_shapes(golden):
    g = golden("performance_T3L2_n4_16")
    Tl, L, n0, C, *size = [int(v) for v in g["cfg"]]
    assert (Tl, L, n0, C, size) == (3, 2, 4, 5, [16, 16, 16])
    assert list(g["metrics"]) == METRICS
    assert g["seg_x"].dtype == np.uint8 and g["seg_x"].shape == (1, 1, 16, 16, 16) == g["seg_y"].shape
    assert int(g["seg_x"].max()) < C and int(g["seg_y"].max()) < C
    assert g["lm_x"].shape == (1, 6, 3) == g["lm_y"].shape
    for case in "ab":
        for m in METRICS:
            v = g[f"{case}.{m}"]
            assert v.shape == (L,) and v.dtype == np.float64 and np.isfinite(v).all(), (case, m)
        assert (g[f"{case}.LM_MAE"][1:] == 0).all() and (g[f"{case}.LM_Euclid"][1:] == 0).all()        # evaluate.py:1461, 1470
        assert g[f"{case}.LM_MAE"][0] > 0 and g[f"{case}.LM_Euclid"][0] > 0
        assert ((g[f"{case}.Dice"] > 0) & (g[f"{case}.Dice"] < 1)).all()
        for l, s in enumerate((16, 4) if case == "a" else (16, 8)):          # T3 / L2: level 1 of the model lives on 4^3
            assert g[f"{case}.jdet.{l}"].shape == (1, s, s, s)
    for l, s in enumerate((16, 8)):
        assert g[f"b.outputs.{l}"].shape == (1, 1, s, s, s) and g[f"b.final_dfs.{l}"].shape == (1, 3, s, s, s)
        # the stored scalars are the stored maps': folding occurs, and no determinant sits within rounding of zero
        jd = g[f"b.jdet.{l}"]
        assert abs(100.0 * (jd <= 0).sum() / jd.size - g["b.JDetLeq0"][l]) < 1e-4 and g["b.JDetLeq0"][l] > 1.0
        assert abs(jd.astype(np.float64).std(ddof=1) - g["b.JDetStd"][l]) <= 1e-5 * g["b.JDetStd"][l]
    assert g["b.y"].shape == (1, 1, 16, 16, 16)


def test_performance_table_aggregation():
    """nanmean with zeros as missing over 2 loaders of unequal length, LM metrics zero above level 0, a metric one loader never has;
    columns ordered as np.repeat(loader_names, num_metrics) / np.tile(metric_names, num_datasets) (evaluate.py:1486-1488)"""
    from pulpo_amd.evaluation import PerformanceTable
    names, loaders, L, n_inputs = ["RMSE", "Dice", "LM_MAE"], ["oasis", "brats"], 3, 4
    table = PerformanceTable(names, L, loaders, n_inputs)
    all_metrics = np.zeros((len(names), L, len(loaders), n_inputs))
    rng = np.random.default_rng(1)
    for k, n_in in enumerate((4, 2)):
        for j in range(n_in):
            scores = {"RMSE": {l: torch.tensor(float(rng.uniform(0.1, 1.0))) for l in range(L)},
                      "LM_MAE": {l: torch.tensor(float(rng.uniform(1.0, 3.0)) if l == 0 else 0.0) for l in range(L)}}
            if k == 0:                                           # only the first loader has segmentations
                scores["Dice"] = {l: torch.tensor(float(rng.uniform(0.2, 0.9)), dtype=torch.float64) for l in range(L)}
            table.add(k, j, scores)
            for h, m in enumerate(names):
                for l, v in scores.get(m, {}).items():
                    all_metrics[h, l, k, j] = float(v)
    data, (sets, mets) = table.mean()
    all_metrics[all_metrics == 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = np.concatenate(np.nanmean(all_metrics, axis=-1).T, axis=1)
    assert data.shape == (L, len(loaders) * len(names))
    np.testing.assert_array_equal(data, ref)
    assert list(sets) == ["oasis"] * 3 + ["brats"] * 3 and list(mets) == names * 2
    assert np.isnan(data[1:, 2]).all() and np.isnan(data[:, 4]).all() and np.isfinite(data[:, [0, 1, 3]]).all()
    np.testing.assert_allclose(data[0, 3], np.mean([all_metrics[0, 0, 1, j] for j in range(2)]))           # the unfilled slots do not count
    # an empty table is all-missing, not an error
    empty, _ = PerformanceTable(names, L, loaders, n_inputs).mean()
    assert empty.shape == (L, 6) and np.isnan(empty).all()


def test_performance_table_argument_errors():
    from pulpo_amd.evaluation import PerformanceTable
    with pytest.raises(ValueError):
        PerformanceTable([], 2, ["a"], 1)
    with pytest.raises(ValueError):
        PerformanceTable(["RMSE"], 0, ["a"], 1)
    table = PerformanceTable(["RMSE"], 2, ["a"], 2)
    one = {"RMSE": {0: torch.tensor(1.0)}}
    with pytest.raises(IndexError):
        table.add(1, 0, one)
    with pytest.raises(IndexError):
        table.add(0, 2, one)
    with pytest.raises(IndexError):
        table.add(0, 0, {"RMSE": {2: torch.tensor(1.0)}})
    with pytest.raises(KeyError):
        table.add(0, 0, {"Dice": {0: torch.tensor(1.0)}})


def test_landmark_metrics_are_the_harness_expressions():
    """lm_mae: torch.median, the LOWER median of the Manhattan distances (evaluate.py:355-366); lm_euclid: the mean distance (:368-379)"""
    from pulpo_amd import eval_metrics
    a = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 0.0, 0.0], [0.0, 3.0, 4.0]]])
    b = torch.zeros(1, 4, 3)
    assert float(eval_metrics.lm_mae(a, b)) == 2.0               # distances 0, 3, 2, 7: the lower of the two middle values
    np.testing.assert_allclose(float(eval_metrics.lm_euclid(a, b)), (0.0 + 3 ** 0.5 + 2.0 + 5.0) / 4, rtol=1e-6)


def test_level_scores_argument_errors_and_no_cpu_path():
    from pulpo_amd._lib import PulpoHipError
    from pulpo_amd.evaluation import affine_scores, level_scores
    out, df, y = {0: torch.zeros(1, 1, 4, 4, 4)}, {0: torch.zeros(1, 3, 4, 4, 4)}, torch.zeros(1, 1, 4, 4, 4)
    seg = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        level_scores(out, {1: df[0]}, y)
    with pytest.raises(ValueError):
        level_scores(out, df, y, seg_x=seg)
    with pytest.raises(ValueError):
        level_scores(out, df, y, lm_x=torch.zeros(1, 2, 3))
    with pytest.raises(PulpoHipError):                           # operators run on the GPU only: no quiet CPU path
        level_scores(out, df, y)
    with pytest.raises(PulpoHipError):
        affine_scores(y, y)


def test_new_entry_points_size_queries():
    from pulpo_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pulpo_field_quality", "pulpo_field_quality_blocks", "pulpo_field_quality_ws_bytes", "pulpo_warp_labels_soft_dice"):
        assert name in protos, name
    # rows of W voxels, lanes-per-row the power of two that wastes the fewest lanes: 160 -> 32 lanes, 8 rows per 256-thread block
    assert lib.query("pulpo_field_quality_blocks", 1, 16, 16, 16) == 16 * 16 // 16
    assert lib.query("pulpo_field_quality_blocks", 1, 160, 160, 160) == 1024
    assert lib.query("pulpo_field_quality_blocks", 1, 1, 24, 20) == 3                # 32 lanes per row, 8 rows per block
    assert lib.query("pulpo_field_quality_ws_bytes", 1, 16, 16, 16) == 16 * 24
    assert lib.query("pulpo_field_quality_blocks", 0, 1, 1, 1) == 0
