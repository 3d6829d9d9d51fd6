"""How the streaming driver's three streams hand work to each other and to the host (REBVIO_HIP_HANDOVER).

Default: the track stream records no event - harvest reads the successor pair's record stamp, a pair's old map goes back to the
pool with a token (the number of pairs whose records the host has to have read) - and a map reused before its token was observed
gets one event there and then. REBVIO_HIP_HANDOVER=events: one event per group of pairs, event-based harvest and release. Either
way only packets move: the records are the per-pair API's, bit for bit, in order. 192x144 stream, 40 frames back and forth over
its 12. (Waits on completed events are not skipped by the library: the runtime drops them itself, tools/handover_probe.hip.)"""
import time

import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import rec, record_words, same_records, set_forms

pytestmark = pytest.mark.gpu

KW = dict(keylines_ref=1500, keylines_max=2500, global_min_matches_threshold=100)
TS = 50000
K_SLOTS = 16   # kPairSlots (rebvio_amd/csrc/common.hpp): the queue holds at most K_SLOTS - 1 pairs
STREAMS = ("track", "scan", "keyline")


def _order(frames, n=40):
    from rebvio_amd import synth
    return synth.pingpong_indices(len(frames), n)


def _device_sync():
    import torch
    torch.cuda.synchronize()


def _stream(B, monkeypatch, stream, handover, lead, group, n=40, sync_every=0, flush_at=(), sync_at=(), before_flush=None, **params):
    """order[:n] through the streaming driver and a flush: (every pair's words + keyline count in order, the hand-over counters, pairs
    started). sync_every k: the device is synchronised after every k-th push; sync_at: before these pushes; flush_at: a flush
    before these pushes, its records taken in order; before_flush(ctx, dev, npx): called between the last push and the last flush."""
    frames, cam = stream
    set_forms(monkeypatch, REBVIO_HIP_HANDOVER=handover, REBVIO_HIP_LEAD=lead, REBVIO_HIP_GROUP=group)
    ctx = B.Context(params_for(B, cam, **dict(KW, **params)))
    dev = ctx.upload_frames(frames)
    npx = cam.width * cam.height
    got = []
    for k, i in enumerate(_order(frames, n)):
        if k in flush_at:
            got.extend(rec(o, m) for o, m in ctx.flush())
        if k in sync_at:
            _device_sync()
        out, m = ctx.push_frame_u8_device(dev + int(i) * npx, k * TS)
        if out.status >= 0:
            got.append(rec(out, m))
        if sync_every and (k + 1) % sync_every == 0:
            _device_sync()
    if before_flush:
        before_flush(ctx, dev, npx)
    got.extend(rec(o, m) for o, m in ctx.flush())
    counters, pairs = ctx.handover_counters(), ctx.pairs_started()
    ctx.close()
    return got, counters, pairs


@pytest.fixture(scope="module")
def per_pair(B, small_stream):
    """the 39 pairs' record words through the per-pair API (computed once, read only)"""
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW))
    maps, out = [], []
    for k, i in enumerate(_order(frames)):
        maps.append(ctx.detect_u8(frames[i], k * TS))
        if len(maps) > 2:
            maps.pop(0).release()
        if k:
            out.append(record_words(ctx.track_pair(maps[0], maps[1])))
    ctx.close()
    assert len(out) == 39 and sum(int(w[-1]) == 0 for w in out) >= 30   # (status is the record's last word: the pairs track)
    return out


def _same_as_per_pair(got, per_pair, what):
    same_records([w[:-1] for w in got], per_pair, what)


@pytest.mark.parametrize("lead,group", [(3, 1), (5, 4), (12, 6)])
def test_records_are_bit_identical_in_both_hand_overs_and_to_the_per_pair_api(B, small_stream, per_pair, monkeypatch, lead, group):
    ev, c_ev, pairs = _stream(B, monkeypatch, small_stream, "events", lead, group)
    st, c_st, _ = _stream(B, monkeypatch, small_stream, None, lead, group)
    print("events:", c_ev, "\ndefault:", c_st)
    assert pairs == 39 and len(ev) == len(st) == 39
    same_records(st, ev, "default against events")
    _same_as_per_pair(st, per_pair, "default against the per-pair API")
    # events: no wait left out, at least one event per full group; default: no pair and no group records one - only a map reused
    # early does, and the flush that hands the stream's newest map back to the pool
    assert all(c_ev[s]["skipped"] == 0 for s in STREAMS) and c_ev["reuse_fallbacks"] == 0
    assert c_st["scan"] == c_ev["scan"]   # (the detect side's own waits and records are the same)
    assert -(-39 // group) <= c_ev["track"]["events"] <= 39 + 1
    assert c_st["track"]["events"] - c_st["reuse_fallbacks"] <= 1, c_st


def test_shallow_mode_gives_the_same_records_with_fewer_events_than_pairs(B, small_stream, per_pair, monkeypatch):
    """A caller that synchronises the device keeps the driver in its shallow branch (pairs queued alone): after every push, after
    every third, never. Same records in the same order; the default hand-over records fewer track-stream events than pairs."""
    for sync_every in (1, 3, 0):
        got, c, pairs = _stream(B, monkeypatch, small_stream, None, 5, 4, sync_every=sync_every)
        print("sync_every", sync_every, c)
        _same_as_per_pair(got, per_pair, f"synchronised every {sync_every}")
        assert pairs == 39 and c["track"]["events"] < pairs, (sync_every, c)
    # a flush in the middle ends one stream and starts another (the pair across it is not tracked): 20 + 18 records, none lost or
    # duplicated, the same in both hand-overs; the first stream's are the unflushed run's
    st, _, _ = _stream(B, monkeypatch, small_stream, None, 5, 4, flush_at=(21,))
    ev, _, _ = _stream(B, monkeypatch, small_stream, "events", 5, 4, flush_at=(21,))
    assert len(st) == 38
    same_records(st, ev, "flush in the middle")
    same_records([w[:-1] for w in st[:19]], per_pair[:19], "up to the flush's last pair")


def test_both_branches_of_a_map_reuse_are_taken(B, small_stream, per_pair, monkeypatch):
    """Lead 3, single pairs, a small pool: what is left of "both branches of every skipped wait" - the library skips no wait on an
    event (the runtime does), only the keyline stream's wait for the previous life of the map it reuses, by the map's token.

    Token observed, no wait: the device is synchronised before pushes 10, 11, 20 and 21 - the push after a synchronised one has read
    every record there was, so the maps it may reuse are proven idle. Token not observed, the fall-back: behind the last push the
    caller detects nineteen more frames, which takes every free map of the pool (lead + group + K_SLOTS + 1 = 21 maps, two held by
    the driver) oldest release first - the last is the old map of the pair queued last, whose token cannot have been observed: its
    successor is not queued yet. One event is recorded on the track stream there and the keyline stream waits for it. Nothing here depends on
    how fast the device is. The records are the per-pair API's.

    Then the same frames enlarged eight times (1536x1152), where a detection takes the device several pushes' time and the host runs
    ahead of it (at 192x144 it is the other way round): the records of the two hand-overs agree there too."""
    from support import enlarged_stream
    held = []

    def detect_more(ctx, dev, npx):
        before = ctx.handover_counters()
        for j in range(3 + 1 + K_SLOTS + 1 - 2):
            held.append(ctx.detect_u8_device(dev + (j % 12) * npx, (100 + j) * TS))
        after = ctx.handover_counters()
        assert after["reuse_fallbacks"] > before["reuse_fallbacks"] and after["track"]["events"] > before["track"]["events"]
        for m in held:
            m.release()

    got, c, pairs = _stream(B, monkeypatch, small_stream, None, 3, 1, sync_at=(10, 11, 20, 21), before_flush=detect_more, map_pool=4)
    print(c)
    assert pairs == 39
    _same_as_per_pair(got, per_pair, "lead 3, small pool, maps reused early")
    assert c["keyline"]["skipped"] >= 1 and c["reuse_fallbacks"] >= 1, c
    assert c["track"]["skipped"] == c["scan"]["skipped"] == 0
    big = enlarged_stream(1536, 1152, 12, factor=8)
    kw = dict(keylines_ref=12000, keylines_max=16000, map_pool=4)
    st, c, pairs = _stream(B, monkeypatch, big, None, 3, 1, **kw)
    ev, c_ev, _ = _stream(B, monkeypatch, big, "events", 3, 1, **kw)
    print(c, "\nevents:", c_ev, "\nstatus", [int(w[-2]) for w in st])
    assert pairs == 39 and len(st) == 39
    same_records(st, ev, "enlarged frames, default against events")


def test_forged_stamp_ends_in_minus_12_without_a_time_out(B, small_stream, monkeypatch):
    """rebvio_hip_test_forge_record_stamp before frame 8. The forged pair's stamp never arrives, so no pair behind it is reported;
    the call that has to BLOCK finds the track stream idle, looks once more and answers -12: the push that needs a result slot
    (K_SLOTS - 1 pairs queued), or the flush of a 12-frame stream."""
    from rebvio_amd import backend
    frames, cam = small_stream
    npx = cam.width * cam.height
    set_forms(monkeypatch, REBVIO_HIP_HANDOVER=None, REBVIO_HIP_LEAD=None, REBVIO_HIP_GROUP=None)
    for n, where in ((40, "push"), (12, "flush")):
        ctx = B.Context(params_for(B, cam, **KW))
        dev = ctx.upload_frames(frames)
        failed_at, records = None, 0
        t0 = time.monotonic()
        with pytest.raises(backend.HipError) as e:
            for k, i in enumerate(_order(frames, n)):
                if k == 8:
                    backend._chk(backend.lib().rebvio_hip_test_forge_record_stamp(ctx.h))
                failed_at = k
                records += ctx.push_frame_u8_device(dev + int(i) * npx, k * TS)[0].status >= 0
            failed_at = "flush"
            ctx.flush()
        dt = time.monotonic() - t0
        started = ctx.pairs_started()
        ctx.close()
        print(where, "failed at", failed_at, "pairs started", started, "records before", records, f"{dt:.3f} s")
        assert "error -12" in str(e.value), str(e.value)
        if where == "push":
            assert failed_at != "flush" and started >= K_SLOTS - 1 and records < 8, (failed_at, started, records)
        else:
            assert failed_at == "flush", failed_at
        assert dt < 1.0, dt   # (poll_pair_records' two-second limit is not involved: the idle stream decides)


def test_steady_state_allocates_nothing(B, small_stream, monkeypatch):
    frames, cam = small_stream
    npx = cam.width * cam.height
    set_forms(monkeypatch, REBVIO_HIP_HANDOVER=None, REBVIO_HIP_LEAD=None, REBVIO_HIP_GROUP=None)
    ctx = B.Context(params_for(B, cam, **KW))
    dev = ctx.upload_frames(frames)
    live = {}
    for k, i in enumerate(_order(frames, 200)):
        ctx.push_frame_u8_device(dev + int(i) * npx, k * TS)
        if k + 1 in (60, 200):
            live[k + 1] = B.test_live_resources()
    c = ctx.handover_counters()
    ctx.flush()
    ctx.close()
    print(live, c)
    assert live[200] == live[60], live
