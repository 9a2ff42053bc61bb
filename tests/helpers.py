"""Shared test helpers: golden CSV parsing and comparison utilities; the clouds, scenes and poses come from dcreg_amd.scenes."""
import csv
import gzip
import os

import numpy as np

from dcreg_amd.scenes import *                    # noqa: F401,F403  (read_pcd_xyz, cylinder_cloud, scene_*, pose6d_matrix, deg2rad, ...)
from dcreg_amd.scenes import FIXTURE_PCD          # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REPO = os.path.dirname(HERE)


def read_csv_rows(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        return list(csv.DictReader(f))


def golden_rows(family, fname, method=None):
    rows = read_csv_rows(os.path.join(GOLDEN, family, fname))
    if method is not None:
        rows = [r for r in rows if r["Method"] == method]
    return rows


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def single_registration(ctx, frame, T0, method, cfg):
    """the record dcreg_register_frames promises for one frame: dcreg_set_source + dcreg_icp_run (compare with assert_record)"""
    ctx.set_source(frame)
    res, logs = ctx.icp_run(T0, method, cfg)
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    last = logs[-1] if logs else None
    return dict(T=T.reshape(16), iterations=res.iterations, converged=res.converged, status=res.status,
                rmse=last.rmse if last else 0.0, fitness=last.fitness if last else 0.0, corr=last.effective_points if last else 0,
                H=np.array(last.H_upper[:]) if last else np.zeros(21), mask=list(last.analysis.degenerate_mask[:]) if last else [0] * 6,
                trans_err=last.trans_error_vs_gt if last else None)


def assert_record(tr, s, what):
    assert (tr.iterations, tr.converged, tr.status) == (s["iterations"], s["converged"], s["status"]), what
    assert np.array_equal(np.array(tr.final_transform[:]), s["T"]), what
    assert tr.final_rmse == s["rmse"] and tr.final_fitness == s["fitness"] and tr.corr_num == s["corr"], what
    assert np.array_equal(np.array(tr.H_upper[:]), s["H"]) and list(tr.degenerate_mask[:]) == s["mask"], what
