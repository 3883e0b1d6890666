"""cloud_compare(..., normals=...) on a small synthetic pair: a height field as the
truth, dp_fused_point records with known normals as the reconstruction.  The
"normals" entry equals cloud_normal_error fed from the reference's normals
(tests/cloudnormals_ref.py) exactly, and normals=None changes nothing."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

import cloudalign_ref as AR
import cloudnearest_ref as CR
import cloudnormals_ref as NR

pytestmark = pytest.mark.gpu

TAU, RADIUS = 0.05, 0.2


def height(xy):
    return 0.2 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1])


def analytic_normals(xy):
    gx = 0.6 * np.cos(3 * xy[:, 0]) * np.cos(2 * xy[:, 1])
    gy = -0.4 * np.sin(3 * xy[:, 0]) * np.sin(2 * xy[:, 1])
    n = np.stack([-gx, -gy, np.ones(len(xy))], axis=1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(31)
    txy = rng.random((400, 2))
    truth = np.concatenate([txy, height(txy)[:, None]], axis=1).astype(np.float32)
    rxy = rng.random((250, 2)) * 1.1  # some of it beyond the truth
    recon = np.zeros(250, N.FUSED_DTYPE)
    recon["pos"] = np.concatenate([rxy, (height(rxy) + 0.01 * rng.standard_normal(250))[:, None]], axis=1)
    nrm = analytic_normals(rxy) + 0.1 * rng.standard_normal((250, 3))  # known, and a few degrees off
    nrm[::2] *= -1  # the angle is unsigned
    recon["normal"] = nrm
    recon["normal"][3] = 0
    recon["normal"][4] = np.float32([np.nan, 0, 1])
    recon["pos"][5] = np.float32([np.inf, 0, 0])
    return recon, truth, NR.normals(truth, 16, RADIUS)["normal"]


@pytest.fixture(scope="module")
def eng():
    with dp.Engine(device=0) as e:
        yield e


def same(a, b):
    """two entries of numbers, NaN equal to NaN"""
    return a.keys() == b.keys() and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def test_the_normals_entry_is_cloud_normal_error_of_the_reference_normals(eng, pair):
    recon, truth, truth_normals = pair
    got = dp.cloud_compare(eng, recon, truth, TAU, RADIUS, normals=dict(k=16))
    near = CR.nearest(recon, truth, RADIUS)
    want = dp.cloud_normal_error(recon["normal"], truth_normals, near["index"], near["dist"], TAU)
    assert same(got["normals"], want) and same(want, NR.normal_error(recon["normal"], truth_normals, near["index"],
                                                                      near["dist"], TAU))
    # not vacuous: most of the reconstruction counts, the error is the planted few degrees
    assert 150 < want["n"] <= got["accuracy"]["within_tau"] and 1 < want["median_deg"] < 15
    assert want["median_deg"] <= want["p90_deg"] < 45
    # another k and radius for the truth's normals: another answer
    other = dp.cloud_compare(eng, recon, truth, TAU, RADIUS, normals=dict(k=6, max_dist=0.1))
    tn = NR.normals(truth, 6, 0.1)["normal"]
    assert same(other["normals"], dp.cloud_normal_error(recon["normal"], tn, near["index"], near["dist"], TAU))
    assert other["normals"]["mean_deg"] != want["mean_deg"]


def test_without_the_argument_nothing_changes(eng, pair):
    recon, truth, _ = pair
    plain = dp.cloud_compare(eng, recon, truth, TAU, RADIUS)
    none = dp.cloud_compare(eng, recon, truth, TAU, RADIUS, normals=None)
    with_normals = dp.cloud_compare(eng, recon, truth, TAU, RADIUS, normals={})
    assert sorted(plain) == sorted(none) == ["accuracy", "completeness", "fscore"]
    for name in ("accuracy", "completeness"):
        assert same(plain[name], none[name]) and same(plain[name], with_normals[name])
    assert plain["fscore"] == none["fscore"] == with_normals["fscore"]
    with pytest.raises(ValueError):
        dp.cloud_compare(eng, recon["pos"], truth, TAU, RADIUS, normals={})  # no normal field


def test_with_align_the_normals_turn_with_the_records(eng, pair):
    recon, truth, truth_normals = pair
    # the reconstruction in a frame of its own: turned by 5 degrees about z and shifted
    c, s = np.cos(np.radians(5)), np.sin(np.radians(5))
    M = np.float64([[c, -s, 0, 0.02], [s, c, 0, -0.01], [0, 0, 1, 0.015]])
    away = AR.transform(recon, M, normals=True)
    got = dp.cloud_compare(eng, away, truth, TAU, RADIUS, align=dict(iterations=20), normals={})
    back = AR.transform(away, got["align"]["matrix"], normals=True)
    near = CR.nearest(back, truth, RADIUS)
    want = dp.cloud_normal_error(back["normal"], truth_normals, near["index"], near["dist"], TAU)
    assert same(got["normals"], want) and want["n"] > 100
    # the registration found its way back, so the error is the planted one again
    home = dp.cloud_compare(eng, recon, truth, TAU, RADIUS, normals={})["normals"]
    assert abs(want["median_deg"] - home["median_deg"]) < 2
    # unturned normals would be about 5 degrees worse in the tangent plane: not the same numbers
    stale = dp.cloud_normal_error(away["normal"], truth_normals, near["index"], near["dist"], TAU)
    assert stale["mean_deg"] != want["mean_deg"]
    # the aligned comparison without normals is as before
    plain = dp.cloud_compare(eng, away, truth, TAU, RADIUS, align=dict(iterations=20))
    assert same(plain["accuracy"], got["accuracy"]) and same(plain["completeness"], got["completeness"])


def test_pmvs_evaluate_passes_it_through():
    from densepoints_amd import synth

    cfg = synth.config(4, 160, 120, 1)
    P, imgs, seeds = synth.scene_host(cfg)
    pm = dp.PMVS()
    for v in range(cfg.n_views):
        pm.add_camera(dp.View(P[v], imgs[v]))
    assert pm.run(seeds)
    lo, hi = seeds[:, :2].min(axis=0), seeds[:, :2].max(axis=0)
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 48), np.linspace(lo[1], hi[1], 36), indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1)
    z, _ = synth.surface(cfg, xy)
    truth = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
    tau = float(np.float32(2 * max((hi[0] - lo[0]) / 47, (hi[1] - lo[1]) / 35)))
    plain = pm.evaluate(truth, tau)
    got = pm.evaluate(truth, tau, normals=dict(k=8))
    assert "normals" not in plain and same(plain["accuracy"], got["accuracy"])
    with dp.Engine(device=0) as eng:
        want = dp.cloud_compare(eng, pm.patches, truth, tau, normals=dict(k=8))
    assert same(got["normals"], want["normals"]) and 0 < got["normals"]["n"] <= got["accuracy"]["within_tau"]
    assert 0 <= got["normals"]["median_deg"] <= got["normals"]["p90_deg"] <= 90
    fused = pm.evaluate(truth, tau, cloud="fused", normals={})
    assert fused["normals"]["n"] > 0
    with pytest.raises(ValueError):
        pm.evaluate(truth, tau, cloud=pm.patches["pos"], normals={})
    with pytest.raises(ValueError):
        pm.evaluate(truth, tau, mesh=(np.zeros((3, 3), np.float32), np.int32([[0, 1, 2]])), normals={})
