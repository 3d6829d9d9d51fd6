"""Place recognition above the C-ABI, on the GPU: rebvio::EdgeMap::placeSignature, rebvio::PlaceDb,
rebvio::Rebvio::setPlaceRecognition / registerPlaceCallback (tests/cpp/test_place.cpp says what it checks) and
`rebvio_replay --places`, on a ping-pong stream: 160x120, 19 base frames, 37 frames in all, a keyframe every 3 frames,
exclude_last = 2."""
import os
import subprocess

import pytest

from support import host_lib  # noqa: F401
from support import ROOT

pytestmark = pytest.mark.gpu

W, H, BASE, N, EVERY, EXCLUDE = 160, 120, 19, 37, 3, 2


@pytest.fixture(scope="module")
def stream_file(tmp_path_factory):
    from rebvio_amd import synth
    d = tmp_path_factory.mktemp("place")
    frames, cam = synth.render_stream(W, H, BASE)
    idx = synth.pingpong_indices(BASE, N)
    assert list(idx[:3]) == [0, 1, 2] and idx[N - 1] == 0 and idx[BASE - 1] == BASE - 1
    path = d / "frames.u8"
    frames[idx].tofile(path)
    return d, path, cam


def test_classes_and_callbacks(host_lib, stream_file):
    d, path, cam = stream_file
    exe = str(d / "test_place")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_place.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(path), str(W), str(H), str(N), str(BASE), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", "50",
                        str(EVERY), str(EXCLUDE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


def test_replay_writes_the_places_file(host_lib, stream_file):
    """--places FILE: one line per match, `ts_us tag distance index`; the summary counts queries and matches; the odometry file is
    byte-identical with and without it"""
    d, path, cam = stream_file
    odo0, odo1, places = d / "odometry0.txt", d / "odometry1.txt", d / "places.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(path), "--size", str(W), str(H), "--camera", repr(cam.fm), repr(cam.cx),
            repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r0 = subprocess.run(base + ["--out", str(odo0)], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "place_queries" not in r0.stderr, (r0.stdout, r0.stderr[-2000:])
    r = subprocess.run(base + ["--out", str(odo1), "--places", str(places), "--place-exclude", str(EXCLUDE), "--kf-every", str(EVERY)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert open(odo1, "rb").read() == open(odo0, "rb").read() and len(open(odo0).read().splitlines()) == N - 1
    lines = [ln.split() for ln in open(places).read().splitlines()]
    summary = dict(kv.split("=") for ln in r.stderr.splitlines() if ln.startswith("place_queries=") for kv in ln.split())
    assert int(summary["place_matches"]) == len(lines) and int(summary["place_misses"]) == 0, (summary, len(lines))
    assert int(summary["place_queries"]) >= (N - 1) // EVERY - 1, summary
    assert lines, "a stream that comes back over its own frames has matches under the default max_distance"
    for ln in lines:
        assert len(ln) == 4, ln
        ts, tag, dist, index = (int(v) for v in ln)
        assert ts % 50000 == 0 and tag % 50000 == 0 and tag < ts and 0 <= dist <= 32768 and 0 <= index < int(summary["place_queries"]), ln
    for bad in (["--places"], ["--places", str(places), "--place-exclude", "-1"], ["--places", str(places), "--places", str(places)]):
        b = subprocess.run(base + ["--out", str(odo1)] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode in (1, 2), (bad, b.returncode, b.stderr[-500:])
