"""densify --refine-maps: the CLI's refined depth and score maps and its fused
cloud equal Engine.render_maps -> refine_maps (-> fuse_maps) on the same store
byte for byte; without the flag the outputs are those of the plain chain."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp

from test_cli import run
from test_gpu_parity import SceneCase

pytestmark = pytest.mark.gpu


def test_cli_refine_maps(tmp_path):
    d = str(tmp_path / "scene")
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    base = ("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o",
            str(tmp_path / "points.ply"), "--filter")
    maps_dir, fused = tmp_path / "maps", tmp_path / "fused.ply"
    report = json.loads(run(*base, "--depth-maps", str(maps_dir), "--depth-normals", "--fuse", str(fused),
                            "--refine-maps", "1", "--refine-window", "5", "--refine-min-ncc", "0.4").stdout)
    sc = SceneCase(V=4, W=160, H=120, kind=1)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        store, _ = eng.densify(sc.seeds)
        store = store[eng.filter_patches(store) == 1]
        maps = eng.render_maps(store, normals=True)
        ref = eng.refine_maps(maps["depth"], maps["normal"], window=5, min_ncc=0.4)
        pts, _ = eng.fuse_maps(ref["depth"], ref["normal"])
        plain, _ = eng.fuse_maps(maps["depth"], maps["normal"])
    assert ref["stats"]["moved"] > 0 and ref["stats"]["kept"] > 0
    for v in range(4):
        for name, want in (("depth", ref["depth"][v]), ("score", ref["score"][v]), ("normal", ref["normal"][v])):
            got = dp.read_pfm(str(maps_dir / ("%s_%04d.pfm" % (name, v))))
            assert got.tobytes() == want.tobytes(), (name, v)
    want_ply = tmp_path / "ref.ply"
    dp.write_ply(str(want_ply), pts)
    assert fused.read_bytes() == want_ply.read_bytes()
    for key in ("refined_maps", "refined"):
        r = report[key]
        assert (r["passes"], r["kept"], r["moved"], r["filled"]) == (1, ref["stats"]["kept"], ref["stats"]["moved"],
                                                                      ref["stats"]["filled"])
        assert r["refine_ms"] > 0
    assert report["fused"]["points"] == len(pts) > 0
    # without the flag: the plain chain, no score maps, no report members
    maps2, fused2 = tmp_path / "maps2", tmp_path / "fused2.ply"
    report = json.loads(run(*base, "--depth-maps", str(maps2), "--fuse", str(fused2)).stdout)
    assert "refined" not in report and "refined_maps" not in report
    assert not (maps2 / "score_0000.pfm").exists()
    assert dp.read_pfm(str(maps2 / "depth_0000.pfm")).tobytes() == maps["depth"][0].tobytes()
    plain_ply = tmp_path / "plain.ply"
    dp.write_ply(str(plain_ply), plain)
    assert fused2.read_bytes() == plain_ply.read_bytes() != fused.read_bytes()
    # two passes feed the first one's output back in
    json.loads(run(*base, "--depth-maps", str(maps2), "--refine-maps", "2", "--refine-window", "5",
                   "--refine-min-ncc", "0.4").stdout)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        two = eng.refine_maps(ref["depth"], ref["normal"], window=5, min_ncc=0.4)
    assert dp.read_pfm(str(maps2 / "depth_0002.pfm")).tobytes() == two["depth"][2].tobytes()
    assert np.any(two["depth"][2] != ref["depth"][2])
    # bad values are refused with a message
    for bad in (("--refine-maps", "65"), ("--refine-maps", "x"), ("--refine-window", "4"), ("--refine-window", "13"),
                ("--refine-min-ncc", "1.5"), ("--refine-min-ncc", "nan")):
        r = run("-i", os.path.join(d, "scene.json"), *bad, check=False)
        assert r.returncode == 2 and "expects" in r.stderr
