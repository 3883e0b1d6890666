"""programs/densify (the C++ CLI over the C ABI): scene JSON, image decoding,
seeds and settings on the CPU; the full run (dp_densify -> PLY) on the GPU,
byte-compared with the oracle's densify written in PrintCloud format."""
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from densepoints_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "programs", "densify", "densify")


def fnv(bgr: np.ndarray) -> str:
    h = 1469598103934665603
    for b in np.ascontiguousarray(bgr, dtype=np.uint8).ravel().tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def run(*args, check=True):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)
    if check and r.returncode != 0:
        raise AssertionError(f"densify {args} -> {r.returncode}: {r.stderr}")
    return r


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("scene"))
    out = json.loads(run("--synthetic", "4,160,120,1", "--write-scene", d).stdout)
    assert out["views"] == 4
    return d


def test_synthetic_scene_roundtrip(scene_dir):
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    with open(os.path.join(scene_dir, "scene.json")) as f:
        sc = json.load(f)
    assert sc["imagesPath"] == scene_dir and len(sc["views"]) == 4
    for v, view in enumerate(sc["views"]):
        assert np.array_equal(np.array(view["projectionMatrix"]), P[v])  # %.17g round trip is exact
    seeds = np.loadtxt(os.path.join(scene_dir, "seeds.xyz")).reshape(-1, 3)
    assert np.array_equal(seeds, synth.seeds(cfg, P))
    chk = json.loads(run("-i", os.path.join(scene_dir, "scene.json"), "--seeds",
                         os.path.join(scene_dir, "seeds.xyz"), "--check-only").stdout)
    assert chk["views"] == 4 and chk["width"] == 160 and chk["height"] == 120
    assert chk["seeds"] == len(seeds)
    assert chk["image_fnv"] == [fnv(synth.render_host(cfg, P, v)) for v in range(4)]


def _png(path, px: np.ndarray, ctype: int):
    """Minimal PNG encoder exercising every filter type (row y uses filter y % 5)."""
    h, w = px.shape[:2]
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    a = px.reshape(h, w * ch).astype(np.int32)
    raw = bytearray()
    for y in range(h):
        f = y % 5
        row = a[y]
        up = a[y - 1] if y else np.zeros_like(row)
        left = np.concatenate([np.zeros(ch, np.int32), row[:-ch]])
        ul = np.concatenate([np.zeros(ch, np.int32), up[:-ch]])
        if f == 0:
            out = row
        elif f == 1:
            out = row - left
        elif f == 2:
            out = row - up
        elif f == 3:
            out = row - (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
            out = row - pred
        raw.append(f)
        raw += (out & 255).astype(np.uint8).tobytes()

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(bytes(raw), 6)))
        f.write(chunk(b"IEND", b""))


def test_png_decoding_all_filters_and_colour_types(tmp_path):
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (37, 53, 1), dtype=np.uint8)], axis=2)
    gray = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    _png(tmp_path / "rgb.png", rgb, 2)
    _png(tmp_path / "rgba.png", rgba, 6)
    _png(tmp_path / "gray.png", gray, 0)
    P = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]]
    scene = {"imagesPath": str(tmp_path),
             "views": [{"filename": n, "projectionMatrix": P} for n in ("rgb.png", "rgba.png", "gray.png")]}
    (tmp_path / "scene.json").write_text(json.dumps(scene))
    (tmp_path / "seeds.xyz").write_text("# x y z\n0 0 1\n0.5 0.25 2\n")
    chk = json.loads(run("-i", str(tmp_path / "scene.json"), "--seeds", str(tmp_path / "seeds.xyz"),
                         "--check-only").stdout)
    bgr = rgb[:, :, ::-1]  # cv::imread order; alpha dropped; gray replicated
    assert chk["seeds"] == 2
    assert chk["image_fnv"] == [fnv(bgr), fnv(bgr), fnv(np.repeat(gray[:, :, None], 3, axis=2))]


def test_bad_inputs_fail_loudly(tmp_path, scene_dir):
    (tmp_path / "s.json").write_text('{"expand_cell_size": 11, "no_such_option": 1}')
    r = run("-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"),
            "-s", str(tmp_path / "s.json"), "--check-only", check=False)
    assert r.returncode == 1 and "no_such_option" in r.stderr
    (tmp_path / "ok.json").write_text('{"expand_cell_size": 11, "nm_step": [0.02, 0.2, 0.2]}')
    run("-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"),
        "-s", str(tmp_path / "ok.json"), "--check-only")
    (tmp_path / "bad.json").write_text('{"imagesPath": "x", "views": [ {"filename": 3} ]}')
    r = run("-i", str(tmp_path / "bad.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"), "--check-only",
            check=False)
    assert r.returncode == 1
    assert run(check=False).returncode == 2  # no arguments: usage


def test_usage_errors_and_help_exit_codes():
    """an option whose value is missing and an unknown flag: the usage text and
    exit code 2; --synthetic without --write-scene: a message and exit code 1;
    -h: the usage text on stderr and exit code 0"""
    for bad in (("-i",), ("--no-such-flag",)):
        r = run(*bad, check=False)
        assert r.returncode == 2 and r.stderr.startswith("usage: densify -i scene.json") and r.stdout == ""
    r = run("--synthetic", "2,32,24,0", check=False)
    assert r.returncode == 1 and r.stderr == "densify: --synthetic needs --write-scene DIR\n" and r.stdout == ""
    r = run("-h", check=False)
    assert r.returncode == 0 and r.stderr.startswith("usage: densify -i scene.json") and r.stdout == ""


@pytest.mark.gpu
def test_cli_level_1_ply_equals_python_path(scene_dir, tmp_path):
    """densify --level 1: the context set-up's pyramid branch (dp_build_pyramid(2),
    dp_set_level(1)); the PLY equals write_ply of the same calls made through
    the Python Engine, byte for byte."""
    import densepoints_amd as dp
    from densepoints_amd.pmvs import write_ply

    out = tmp_path / "points.ply"
    res = json.loads(run("-i", os.path.join(scene_dir, "scene.json"), "--seeds",
                         os.path.join(scene_dir, "seeds.xyz"), "--level", "1", "-o", str(out)).stdout)
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    with dp.Engine(device=0) as eng:
        eng.set_views([dp.View(P[v], synth.render_host(cfg, P, v)) for v in range(4)])
        eng.build_pyramid(2)
        eng.set_level(1)
        patches, st = eng.densify(synth.seeds(cfg, P))
    assert res["patches"] == len(patches) > 0
    ref = tmp_path / "python.ply"
    write_ply(str(ref), patches)
    assert out.read_bytes() == ref.read_bytes()
    full = tmp_path / "level0.ply"
    run("-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"), "-o", str(full))
    assert out.read_bytes() != full.read_bytes()  # the level took effect


@pytest.mark.gpu
def test_cli_missing_device_exits_1(scene_dir):
    """a device that does not exist: dp_ctx_create's argument error, returned
    after the scene is loaded and before any kernel runs"""
    r = run("-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"),
            "--device", "9999", check=False)
    assert r.returncode == 1 and "dp_ctx_create failed" in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_cli_rccl_on_a_shared_device_exits_1(scene_dir):
    """--exchange rccl with two contexts wrapped onto one device: the exchange
    refuses before any kernel runs, and both contexts are released"""
    from densepoints_amd._native import lib

    if lib.dp_device_count() != 1:
        pytest.skip("--gpus 2 wraps onto one device only where one device is exposed")
    r = run("-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"),
            "--gpus", "2", "--exchange", "rccl", "--device", "0", check=False)
    assert r.returncode == 1 and "--exchange rccl needs one device per context" in r.stderr


@pytest.mark.gpu
def test_cli_densify_ply_equals_oracle(scene_dir, tmp_path, orc):
    from densepoints_amd.pmvs import write_ply

    out = tmp_path / "points.ply"
    res = json.loads(run("-i", os.path.join(scene_dir, "scene.json"), "--seeds",
                         os.path.join(scene_dir, "seeds.xyz"), "-o", str(out)).stdout)
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    imgs = [synth.render_host(cfg, P, v) for v in range(4)]
    S = orc.Scene(P, imgs)
    op, ost = S.densify(synth.seeds(cfg, P))
    assert res["patches"] == ost["patches"] > 0
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert out.read_bytes() == ref.read_bytes()


@pytest.mark.gpu
def test_cli_fast_mode_ply_equals_oracle(scene_dir, tmp_path, orc):
    """densify --mode fast: the performance-mode densify (dp_fast_options.densify)
    through the CLI; the PLY equals the oracle's generation-at-a-time restatement
    with the fast refine, byte for byte, on one GPU and partitioned over two
    contexts (--gpus 2)."""
    from densepoints_amd import FastOptions
    from densepoints_amd.pmvs import write_ply

    out = tmp_path / "points.ply"
    args = ("-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"))
    res = json.loads(run(*args, "--mode", "fast", "-o", str(out)).stdout)
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    imgs = [synth.render_host(cfg, P, v) for v in range(4)]
    S = orc.Scene(P, imgs)
    op = orc.GenerationEngine(S, threads=8, fast=FastOptions(densify=1)).densify_all(synth.seeds(cfg, P))
    assert res["mode"] == "fast" and res["patches"] == len(op) > 0
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert out.read_bytes() == ref.read_bytes()
    out2 = tmp_path / "points2.ply"
    res2 = json.loads(run(*args, "--mode", "fast", "--gpus", "2", "-o", str(out2)).stdout)
    assert res2["gpus"] == 2 and out2.read_bytes() == ref.read_bytes()
    assert run(*args, "--mode", "turbo", check=False).returncode == 2
    # --fast-gradient 1: the analytic-gradient refine (spec v4)
    out3 = tmp_path / "points3.ply"
    run(*args, "--mode", "fast", "--fast-gradient", "1", "-o", str(out3))
    op3 = orc.GenerationEngine(S, threads=8, fast=FastOptions(densify=1, gradient=1)).densify_all(synth.seeds(cfg, P))
    ref3 = tmp_path / "oracle3.ply"
    write_ply(str(ref3), op3)
    assert out3.read_bytes() == ref3.read_bytes() != ref.read_bytes()


@pytest.mark.gpu
def test_cli_full_pipeline_generates_seeds(tmp_path_factory, tmp_path, orc):
    """densify -i scene.json with no --seeds: PMVS::Run's InsertSeeds
    (Matcher::GenerateSeeds on the device) then expansion; the PLY equals the
    oracle's seed generation + densify, byte for byte."""
    from densepoints_amd.pmvs import write_ply

    d = str(tmp_path_factory.mktemp("scene_gen"))
    run("--synthetic", "4,320,240,0", "--write-scene", d)
    out = tmp_path / "points.ply"
    res = json.loads(run("-i", os.path.join(d, "scene.json"), "--features", "2000", "--fast-threshold", "8",
                         "-o", str(out)).stdout)
    cfg = synth.config(4, 320, 240, 0)
    P = synth.cameras(cfg)
    imgs = [synth.render_host(cfg, P, v) for v in range(4)]
    r = orc.seeds_run(P, imgs, orc.matcher_options(n_features=2000, fast_threshold=8))
    assert res["generated_seeds"] is True and res["seeds"] == len(r["points"]) > 0
    op, ost = orc.Scene(P, imgs).densify(r["points"])
    assert res["patches"] == ost["patches"] > 0
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert out.read_bytes() == ref.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("views", [2, 4])
def test_cli_baseline_cfg1_vga(tmp_path_factory, tmp_path, orc, views):
    """BASELINE config 1 through programs/densify: the 640x480 synthetic plane.
    With 2 views every patch has fewer than 3 visible non-reference views, so
    the reference writes an empty cloud; the 4-view variant's PLY
    equals the oracle's densify byte for byte (main.cpp:12-40, pmvs.cpp:22-43)."""
    from densepoints_amd.pmvs import write_ply

    d = str(tmp_path_factory.mktemp(f"cfg1_{views}"))
    run("--synthetic", f"{views},640,480,0", "--write-scene", d)
    out = tmp_path / "points.ply"
    res = json.loads(run("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"),
                         "-o", str(out)).stdout)
    cfg = synth.config(views, 640, 480, 0)
    P = synth.cameras(cfg)
    imgs = [synth.render_host(cfg, P, v) for v in range(views)]
    op, ost = orc.Scene(P, imgs).densify(synth.seeds(cfg, P))
    assert res["patches"] == ost["patches"]
    if views == 2:
        assert res["patches"] == 0
    else:
        assert res["patches"] > 100
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert out.read_bytes() == ref.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("gpus,extra", [(2, ("--replicate-below", "0")), (3, ("--replicate-below", "0")),
                                        (1, ("--multi", "--exchange", "rccl", "--replicate-below", "0")),
                                        (2, ("--mode", "fast", "--replicate-below", "0")),
                                        (2, ("--replicate-below", "5")), (3, ("--mode", "fast",))])
def test_cli_gpus_partitioned_equals_one_gpu(scene_dir, tmp_path, gpus, extra):
    """densify --gpus N: N contexts (wrapping onto the available devices),
    every generation partitioned by reference-view super-tile on the device,
    each context's accepted candidates compacted into its slot and the slots
    all-gathered device to device (peer copies when contexts share a GPU; the
    RCCL path -- ncclCommInitAll + ncclAllGather in one group -- forced at one
    context with --multi --exchange rccl); with --replicate-below the small
    generations run on every context device-resident instead (hybrid; the
    default bound, 1024 x contexts, replicates every expansion generation of
    this small scene).  The PLY is byte-identical to the 1-GPU run and the
    evaluations are counted once."""
    one, many = tmp_path / "one.ply", tmp_path / "many.ply"
    args = ["-i", os.path.join(scene_dir, "scene.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz")]
    mode = list(extra[extra.index("--mode"):extra.index("--mode") + 2]) if "--mode" in extra else []
    r1 = json.loads(run(*args, *mode, "-o", str(one)).stdout)
    # (RCCL prints its version banner on stdout: the report is the last line)
    rn = json.loads(run(*args, "-o", str(many), "--gpus", str(gpus), *extra).stdout.strip().splitlines()[-1])
    assert rn["gpus"] == gpus and rn["patches"] == r1["patches"] > 0
    assert rn["evals"] == r1["evals"]
    # only accepted candidates crossed: at least every stored patch (every
    # generation exchanged), at most every candidate
    nseeds = len(open(os.path.join(scene_dir, "seeds.xyz")).readlines())
    assert rn["exchanged"] <= r1["candidates"] + nseeds
    if "--replicate-below" in extra and extra[extra.index("--replicate-below") + 1] == "0":
        assert r1["patches"] <= rn["exchanged"]
    else:
        # hybrid: only the partitioned generations' accepted records crossed
        assert 0 < rn["exchanged"] <= r1["patches"]
    assert many.read_bytes() == one.read_bytes()


def _jpeg_scene(scene_dir, tmp_path, quality=92, subsampling=2):
    """The 4-view synthetic scene with its views re-encoded as JPEG (libjpeg-turbo,
    via Pillow) and, beside it, the same scene with PNG views holding exactly the
    pixels libjpeg-turbo decodes those JPEGs to (the decode cv::imread does)."""
    import io

    from PIL import Image

    with open(os.path.join(scene_dir, "scene.json")) as f:
        sc = json.load(f)
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    decoded = []
    jv, pv = [], []
    for v, view in enumerate(sc["views"]):
        bgr = synth.render_host(cfg, P, v)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, format="JPEG", quality=quality,
                                                                    subsampling=subsampling)
        (tmp_path / f"view{v}.jpg").write_bytes(buf.getvalue())
        dec = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[:, :, ::-1])
        decoded.append(dec)
        _png(tmp_path / f"view{v}.png", np.ascontiguousarray(dec[:, :, ::-1]), 2)
        jv.append({"filename": f"view{v}.jpg", "projectionMatrix": view["projectionMatrix"]})
        pv.append({"filename": f"view{v}.png", "projectionMatrix": view["projectionMatrix"]})
    (tmp_path / "scene_jpg.json").write_text(json.dumps({"imagesPath": str(tmp_path), "views": jv}))
    (tmp_path / "scene_png.json").write_text(json.dumps({"imagesPath": str(tmp_path), "views": pv}))
    return decoded


def test_jpeg_scene_loads_libjpeg_turbo_pixels(scene_dir, tmp_path):
    """a scene folder of JPEG views (cv::imread, types.cpp:7-11):
    the CLI's loaded BGR8 planes equal libjpeg-turbo's decode of the same files"""
    decoded = _jpeg_scene(scene_dir, tmp_path)
    chk = json.loads(run("-i", str(tmp_path / "scene_jpg.json"), "--seeds", os.path.join(scene_dir, "seeds.xyz"),
                         "--check-only").stdout)
    assert chk["image_fnv"] == [fnv(d) for d in decoded]


@pytest.mark.gpu
def test_cli_jpeg_scene_ply_equals_png_scene(scene_dir, tmp_path, orc):
    """densify -i scene.json with .jpg views writes the same PLY as with PNG
    views of the same pixels, and that PLY equals the oracle's densify of the
    decoded images, byte for byte."""
    from densepoints_amd.pmvs import write_ply

    decoded = _jpeg_scene(scene_dir, tmp_path)
    seeds = os.path.join(scene_dir, "seeds.xyz")
    oj, op_ = tmp_path / "jpg.ply", tmp_path / "png.ply"
    rj = json.loads(run("-i", str(tmp_path / "scene_jpg.json"), "--seeds", seeds, "-o", str(oj)).stdout)
    rp = json.loads(run("-i", str(tmp_path / "scene_png.json"), "--seeds", seeds, "-o", str(op_)).stdout)
    assert rj["patches"] == rp["patches"] > 0
    assert oj.read_bytes() == op_.read_bytes()
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    op, ost = orc.Scene(P, decoded).densify(synth.seeds(cfg, P))
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert oj.read_bytes() == ref.read_bytes()


@pytest.mark.gpu
def test_cli_flann_matcher_pipeline(tmp_path_factory, tmp_path, orc):
    """densify --matcher flann (MatcherType::FLANN, matcher.cpp:229-240): seeds
    from the FLANN-mode match rule, then the densify; the PLY equals the
    oracle's FLANN-mode seed generation + densify byte for byte."""
    from densepoints_amd.pmvs import write_ply

    d = str(tmp_path_factory.mktemp("scene_flann"))
    run("--synthetic", "4,320,240,0", "--write-scene", d)
    out = tmp_path / "points.ply"
    res = json.loads(run("-i", os.path.join(d, "scene.json"), "--features", "2000", "--fast-threshold", "8",
                         "--matcher", "flann", "-o", str(out)).stdout)
    cfg = synth.config(4, 320, 240, 0)
    P = synth.cameras(cfg)
    imgs = [synth.render_host(cfg, P, v) for v in range(4)]
    r = orc.seeds_run(P, imgs, orc.matcher_options(n_features=2000, fast_threshold=8, matcher_type=1))
    assert res["generated_seeds"] is True and res["seeds"] == len(r["points"]) > 0
    op, ost = orc.Scene(P, imgs).densify(r["points"])
    assert res["patches"] == ost["patches"] > 0
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert out.read_bytes() == ref.read_bytes()
    assert run("-i", os.path.join(d, "scene.json"), "--matcher", "lsh", check=False).returncode == 2


@pytest.mark.gpu
def test_cli_akaze_detector_pipeline(tmp_path_factory, tmp_path, orc):
    """densify --detector akaze (DetectorType::AKAZE, matcher.cpp:56-60,
    166-170): AKAZE seeds, then the densify; the PLY equals the oracle's
    AKAZE seed generation + densify byte for byte."""
    from densepoints_amd.pmvs import write_ply

    d = str(tmp_path_factory.mktemp("scene_akaze"))
    run("--synthetic", "4,320,240,1", "--write-scene", d)
    out = tmp_path / "points.ply"
    res = json.loads(run("-i", os.path.join(d, "scene.json"), "--detector", "akaze", "--akaze-threshold", "0.0002",
                         "-o", str(out)).stdout)
    cfg = synth.config(4, 320, 240, 1)
    P = synth.cameras(cfg)
    imgs = [synth.render_host(cfg, P, v) for v in range(4)]
    r = orc.seeds_run(P, imgs, orc.matcher_options(detector_type=orc.DETECTOR_AKAZE, akaze_threshold=0.0002))
    assert res["generated_seeds"] is True and res["seeds"] == len(r["points"]) > 0
    op, ost = orc.Scene(P, imgs).densify(r["points"])
    assert res["patches"] == ost["patches"] > 0
    ref = tmp_path / "oracle.ply"
    write_ply(str(ref), op)
    assert out.read_bytes() == ref.read_bytes()
    assert run("-i", os.path.join(d, "scene.json"), "--detector", "sift", check=False).returncode == 2
