"""bench.py's self-verification (round 4): the oracle's replay (what a benchmark loop over a resident batch computes),
the per-(shape, front end) traffic record, legs that fail loudly -- on CPU -- and, on the GPU box, the real script at test
size: parity checked AFTER the timed region, the seals' counters in the line, the nvx_group mode, the live path's
latency against the bound INTEGRATION.md states."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import signals

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _line(out):
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_replay_is_one_pipe_fed_the_same_samples_again(nv, oracle):
    """nvxo_replay(loops) == one pipe per stream pushed with the sample `loops` times (state carried), both chains, both
    input rates, both stage-0 forms; nvxo_replay_wide carries the channeliser's 40-sample history the same way."""
    n = 3 * nv.FRAME_IN
    iqs = []
    for s in range(2):
        car = [dict(freq_hz=f, bits=nv.sitor_encode(signals.stream_text(60 + s), 8), bit_offset=101 * (s + 1), phase0=s * 31337, amplitude=6000) for f in (14000, -14000)]
        iqs.append(nv.synth_host(nv.make_stream(car, seed=60 + s, noise_amp=1500), nv.RATE_IN, n))
    iq = np.stack(iqs)
    _s, got = oracle.replay(iq, 2, n, False, 3, 2, 3)
    for k in range(2):
        p = oracle.Pipe(chain_mask=3, charlayer=False)
        for _ in range(3):
            p.push(iq[k])
        assert got[k] == [p.bits(0), p.bits(1)] and len(p.bits(0)) > 200 and len(p.bits(1)) > 200
    # raw rate, one chain, both stage-0 forms
    st, _ = signals.stream_params(nv, 61, nv.RATE_RAW)
    rawiq = nv.synth_host(st, nv.RATE_RAW, 2 * nv.FRAME_RAW)[None]
    for order in (1, 3):
        _s, got = oracle.replay(rawiq, 1, 2 * nv.FRAME_IN, 3 if order == 3 else True, 1, 1, 4)
        p = oracle.Pipe(chain_mask=1, charlayer=False); p.set_stage0(order)
        for _ in range(4):
            p.push_raw(rawiq[0])
        assert got[0] == p.bits(0) and len(got[0]) > 150, order
    # wideband
    rng = np.random.default_rng(3)
    wide = rng.integers(-9000, 9000, size=(1, 2 * nv.FRAME_RAW, 2), dtype=np.int16)
    _s, got = oracle.replay_wide(wide, 1, 2 * nv.FRAME_IN, 2, 3)
    sub = oracle.channelise(np.concatenate([wide[0]] * 3))
    for k in range(8):
        p = oracle.Pipe(chain_mask=3, charlayer=False); p.push(sub[k])
        assert got[2 * k] == p.bits(0) and got[2 * k + 1] == p.bits(1) and len(p.bits(0)) > 100, k


def test_traffic_record_is_per_shape_front_end_and_kernel_source(monkeypatch):
    """roofline.traffic is a static PMC record: quoted only for the (streams, frames, stage-0 order) it was taken on AND only
    while the kernel's sources are the ones it was taken on (an entry carries their hash); otherwise null, with the reason."""
    import bench
    from benchlib import roofline                    # (tools/benchlib: where traffic_record lives and looks its hash function up)
    rec = json.loads((ROOT / "profiles" / "hbm_traffic.json").read_text())
    assert {(e["streams"], e["frames"], e.get("stage0_order", 1)) for e in rec["entries"]} >= {(4096, 12, 1), (4096, 12, 3)}
    for e in rec["entries"]:
        shape = (e["streams"], e["frames"], e.get("stage0_order", 1))
        assert e["bytes_per_launch"] == int(e["fetch_size_kb"] * 1024 * 2 + e["write_size_kb"] * 1024)
        assert 1.0 <= e["bytes_per_launch"] / (4 * e["streams"] * e["frames"] * 645120) < 1.03
        # taken on these sources: quoted ...
        monkeypatch.setattr(roofline, "kernel_source_hash", lambda h=e.get("kernel_source_sha256_16"): h)
        b, src = bench.traffic_record(*shape)
        assert b == e["bytes_per_launch"] and "static" in src
        # ... on others: not
        monkeypatch.setattr(roofline, "kernel_source_hash", lambda: "0123456789abcdef")
        b, why = bench.traffic_record(*shape)
        assert b is None and why.startswith("null") and "kernel sources" in why
    monkeypatch.undo()
    none, why = bench.traffic_record(64, 12, 1)
    assert none is None and why.startswith("null") and "(64, 12, 1)" in why
    assert len(bench.kernel_source_hash()) == 16


def test_a_leg_that_raises_fails_the_run_with_status_4(tmp_path, capsys):
    """finish(): parity false -> status 3 (wins), a leg that raised -> status 4 after the line is printed, else 0."""
    import bench

    class NoRanks:
        dist = None
    line = {"value": 1, "legs_failed": ["variant_a"]}
    with pytest.raises(SystemExit) as e:
        bench.finish(line, True, NoRanks(), 0, leg_errors=True)
    assert e.value.code == 4 and json.loads(capsys.readouterr().out.strip())["legs_failed"] == ["variant_a"]
    with pytest.raises(SystemExit) as e:
        bench.finish(line, False, NoRanks(), 0, leg_errors=True)
    assert e.value.code == 3
    bench.finish(line, True, NoRanks(), 0, leg_errors=False)      # returns


def test_options_of_full_are_refused_in_a_plain_run(monkeypatch, capsys):
    """The options that shape what --full adds (checks, CPU baseline, side legs) end a plain run in the parser (status 2,
    before any GPU call): a command that counted on a check cannot lose it quietly.  With --full they are taken."""
    import bench
    for opts in (["--no-cpu"], ["--verify", "32"], ["--no-legs", "--no-stage0-extra"], ["--after-timed", "128"], ["--cic3-verify", "8"],
                 ["--cpu-streams", "4"], ["--allow-leg-errors"]):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"] + opts)
        with pytest.raises(SystemExit) as e:
            bench.parse()
        err = capsys.readouterr().err.strip().splitlines()[-1]
        assert e.value.code == 2 and "--full" in err and all(o in err for o in opts if o.startswith("--")), (opts, err)
        monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"] + opts)
        assert bench.parse().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", "d"])
    assert not bench.parse().full


def test_dump_outputs_is_a_fixed_sample_in_float_within_64_mb(tmp_path):
    """--dump-outputs: the same seeded sample of streams for the same arguments; every file float32/float64; the bits row of a
    stream is what it decoded after the warm-up (1 = 'B'), the most recent ones when a long run would overrun the 64 MB."""
    import bench

    class StubPipe:                                  # the three calls dump_outputs makes, on made-up results
        def __init__(self, n_bits):
            self.n_bits = n_bits

        def debug_y3(self, s, c):
            return np.full((4 * 288, 2), s + 0.5)

        def bits(self, s, c):
            return ("BY" * self.n_bits)[s % 2:][:self.n_bits]

        def bit_count(self, s, c):
            return self.n_bits

    ids = bench.dump_sample(4096, 4, 30, 288)
    assert np.array_equal(ids, bench.dump_sample(4096, 4, 30, 288)) and len(ids) == 256 and len(set(ids)) == 256
    assert not np.array_equal(ids, np.arange(256)) and 0 <= ids.min() and ids.max() < 4096
    assert np.array_equal(bench.dump_sample(8, 4, 30, 288), np.arange(8))
    bench.dump_outputs(tmp_path / "a", None, StubPipe(100), ids, [40] * len(ids))
    got = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert set(got) == {"y3", "bits", "bit_counts", "stream_ids"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["y3"].shape == (256, 4 * 288, 2) and np.array_equal(got["y3"][:, 0, 0], ids + 0.5)
    assert got["bits"].shape == (256, 60) and np.array_equal(got["stream_ids"], ids) and set(got["bit_counts"]) == {100}
    assert np.array_equal(got["bits"][0], [float(c == "B") for c in StubPipe(100).bits(int(ids[0]), 0)[40:]])
    # a run far too long for the budget: fewer streams, each row the most recent bits, everything under 64 MB
    ids = bench.dump_sample(4096, 4, 100000, 288)
    bench.dump_outputs(tmp_path / "b", None, StubPipe(4 * 32 * 100000), ids, [0] * len(ids))
    assert 1 <= len(ids) < 256 and sum(f.stat().st_size for f in (tmp_path / "b").glob("*.npy")) <= 64 << 20
    bits = np.load(tmp_path / "b" / "bits.npy")
    assert bits.min() >= 0 and bits[0, -1] == float(StubPipe(4 * 32 * 100000).bits(int(ids[0]), 0)[-1] == "B")


def test_self_launch_passes_a_signal_on_to_its_ranks(tmp_path):
    """`bench.py --gpus N` killed by SIGTERM (a driver timeout that is not a process-group kill) must take the ranks
    with it: they run in a session of their own and get the signal passed on."""
    import signal
    worker = tmp_path / "worker.py"
    worker.write_text("import os, sys, time\nopen(sys.argv[1] + '/pid' + os.environ.get('RANK', 'x'), 'w').write(str(os.getpid()))\ntime.sleep(120)\n")
    drv = tmp_path / "drv.py"
    drv.write_text(f"import sys, argparse\nsys.path.insert(0, {str(ROOT)!r})\nimport bench\n"
                   f"bench.self_launch(argparse.Namespace(gpus=2), script={str(worker)!r}, argv=[{str(tmp_path)!r}])\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.Popen([sys.executable, str(drv)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    t0 = time.time()                              # (the first `import torch` of a fresh container can take a minute or two)
    while time.time() - t0 < 300 and p.poll() is None and not ((tmp_path / "pid0").exists() and (tmp_path / "pid1").exists()):
        time.sleep(0.2)
    assert p.poll() is None, p.stderr.read().decode()[-2000:]
    pids = [int((tmp_path / f"pid{r}").read_text()) for r in (0, 1)]
    p.send_signal(signal.SIGTERM)
    assert p.wait(timeout=30) == 128 + signal.SIGTERM
    time.sleep(0.5)
    for pid in pids:
        with pytest.raises(ProcessLookupError):
            os.kill(pid, 0)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_bench_checks_the_timed_launches_and_reports_the_seals():
    """The real bench.py --full at test size with every side leg: parity gated before AND after the timed region, in the
    headline and in each leg; the seals' counters in the line (0 stale hand-overs); no leg failed; exit status 0."""
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--streams", "256", "--frames", "4", "--steps", "5", "--warmup", "2", "--cpu-streams", "8"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = _line(out)
    assert rec["parity"] is True and rec["parity_after_timed"] is True and rec["parity_after_timed_streams"] >= 32 and rec["parity_after_timed_launches"] == 7
    assert rec["roofline"]["handoff"]["stale_detected"] == 0 and rec["roofline"]["handoff"]["launches_failed_integrity"] == 0
    assert rec["legs_failed"] == []
    c3 = rec["stage0_third_order"]
    assert c3["parity"] is True and c3["parity_streams_checked"] == 256 and c3["parity_after_timed"] is True and c3["roofline"]["handoff"]["stale_detected"] == 0
    for leg in ("push_path", "variant_a", "wideband"):
        assert rec[leg]["parity"] is True and rec[leg]["parity_after_timed"] is True and rec[leg]["handoff"]["stale_detected"] == 0, leg
    assert rec["push_path"]["parity_chains_checked"] == 2 * rec["push_path"]["parity_streams_checked"]
    live = rec["live_latency"]
    assert live["parity"] is True
    for name in ("252k", "2016k"):
        st = live["streams"][name]
        assert st["dropped"] == 0 and st["bits_equal_oracle"] and 0 < st["p50_ms"] <= st["p99_ms"] <= st["max_ms"] < 150.0, st


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step_and_repeat_exactly(nv, oracle, tmp_path):
    """bench.py --dump-outputs at test size, twice -- with --full, then plain: the two dumps are identical, file for file,
    so the plain run computes what the checked one does; y3 is the last timed launch's cascade output bit for bit and each
    bits row is what the stream decoded after the warm-up -- the oracle fed the stream's frames warmup + steps times says so."""
    warmup, steps, S, F = 2, 3, 64, 4
    dumps = []
    for run, extra in enumerate((["--full", "--no-cpu", "--no-legs", "--no-stage0-extra", "--after-timed", "32"], [])):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--streams", str(S), "--frames", str(F), "--steps", str(steps),
                              "--warmup", str(warmup), "--dump-outputs", str(d)] + extra,
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        rec = _line(out)
        assert rec["steps"] == steps and rec["warmup"] == warmup and rec["full"] is bool(extra)
        if extra:
            assert rec["parity"] is True
        else:
            assert not {"parity", "cpu_baseline", "legs_failed"} & set(rec)
        dumps.append({f.stem: np.load(f) for f in d.glob("*.npy")})
    a, b = dumps
    assert set(a) == set(b) == {"y3", "bits", "bit_counts", "stream_ids"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    ids = a["stream_ids"].astype(int)
    assert len(ids) == S and a["y3"].shape == (S, F * nv.FRAME_Y3, 2)
    n3 = F * nv.FRAME_Y3
    for k in (0, S // 2, S - 1):
        st, _ = signals.stream_params(nv, int(ids[k]), nv.RATE_RAW)
        buf = nv.DeviceBuffer(F * nv.FRAME_RAW * 4)              # generated the way bench.py generates its batch
        nv.synth_device([st], nv.RATE_RAW, F * nv.FRAME_RAW, buf, F * nv.FRAME_RAW)
        iq = buf.download(F * nv.FRAME_RAW * 4, dtype=np.int16).reshape(-1, 2)
        buf.free()
        ref = oracle.Pipe(chain_mask=1, charlayer=False, tap_y3=(warmup + steps) * n3)
        for _ in range(warmup + steps):
            ref.push_raw(iq)
        assert np.array_equal(a["y3"][k].view(np.uint64), ref.y3(0)[-n3:].view(np.uint64)), f"stream {ids[k]}"
        row = a["bits"][k]
        timed = "".join("B" if v == 1 else "Y" for v in row[row >= 0])
        whole = ref.bits(0)
        assert a["bit_counts"][k] == len(whole) and whole.endswith(timed) and len(timed) > steps * F * 30, f"stream {ids[k]}"


@pytest.mark.gpu
def test_bench_group_mode_two_members_on_one_gpu():
    """`bench.py --gpus 2 --group`: one process, nvx_group over two member handles (both on device 0 here: the first
    multi-GPU box runs the same command without the override), same JSON line, parity before and after the timed region
    per member."""
    env = dict(os.environ, NVX_BENCH_GROUP_DEVICES="0,0")
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--group", "--full", "--streams", "96", "--frames", "6", "--steps", "3", "--warmup", "1"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = _line(out)
    assert rec["n_gpus"] == 2 and rec["parity"] is True and rec["parity_after_timed"] is True
    r = rec["ranks"]
    assert r["backend"] == "group" and r["world_size_seen"] == 2 and r["device_per_rank"] == [0, 0] and r["first_stream_per_rank"] == [0, 96]
    assert r["parity_streams_checked_per_rank"] == [32, 32] and r["parity_after_timed_streams_per_rank"] == [64, 64]
    assert len(r["cascade_avg_launch_ms_per_rank"]) == 2 and all(c > 0 for c in r["cascade_avg_launch_ms_per_rank"])
    assert rec["roofline"]["handoff"]["stale_detected"] == 0 and rec["value"] > 0


@pytest.mark.gpu
def test_nnnn_reaches_add_message_within_the_documented_bound(nv, oracle):
    """a character appears at most 0.32 s (its frame still filling) + launch + collect after
    the per-sample reference (receiver/capt_sched.c:484-528, receiver/nav_b_sm.C:87) would have produced it; the collect
    follows the launch within one wake of the ring's consumer -- the next callback, 50 ms at worst.  A message is fed at
    the real rate through a capture ring; the frame in which it completes is found with the oracle (the first whole-frame
    prefix that yields the message); the sink must have it within 150 ms of that frame's last sample entering the
    callback, i.e. within 0.32 s + 150 ms of any of its samples."""
    from fake_sdr import FakeSdr
    text = "ZCZC LA07\nLATENCY TEST 1234\nNNNN\n"
    st, _ = signals.stream_params(nv, 777, nv.RATE_IN, n_phasing=12, text=text)
    n_frames = 26
    iq = nv.synth_host(st, nv.RATE_IN, n_frames * nv.FRAME_IN)
    k_done = None
    ref = oracle.Pipe(chain_mask=1, charlayer=True)
    for k in range(n_frames):                                # the first frame with which the oracle completes the message
        ref.push(iq[k * nv.FRAME_IN:(k + 1) * nv.FRAME_IN])
        if ref.messages:
            k_done = k + 1; break
    assert k_done is not None and ref.messages[0][1] == "LA07", "the oracle never completed the message"
    with nv.Pipeline(n_streams=1, raw_rate=False, chain_mask=nv.CHAIN_518, max_frames=2, push_mode=True, char_layer=True) as p:
        cap = nv.Capture(p, 0, ring_seconds=2.0)
        sdr = FakeSdr(cap, iq, nv.RATE_IN, nv.FRAME_IN, seed=9, packet=(150, 420))
        sdr.start()
        t_msg = None
        while sdr.is_alive() or t_msg is None:
            if p.messages and t_msg is None:
                t_msg = time.monotonic()
            if not sdr.is_alive() and t_msg is None and time.monotonic() - sdr.frame_done_at[-1] > 1.0:
                break
            time.sleep(0.0005)
        sdr.join()
        lat = cap.latency()
        r, d, c = cap.stats()
        cap.stop()
        assert d == 0 and sdr.late_ms < 50.0, (d, sdr.late_ms)
        assert t_msg is not None and p.messages[0][1:] == ref.messages[0]
        t_frame = sdr.frame_done_at[k_done - 1]              # entry of the callback that carried the deciding frame's last sample
        delay_ms = (t_msg - t_frame) * 1e3
        assert -1.0 <= delay_ms <= 150.0, f"message {delay_ms:.1f} ms after its frame was complete (frame {k_done} of {n_frames})"
        assert lat["frames"] >= n_frames - 2 and lat["max_ms"] < 150.0, lat


@pytest.mark.gpu
def test_the_reference_shaped_surface_at_the_real_rate(nv, oracle, tmp_path):
    """The surface an unmodified capt_sched.c links against (sample_in_1 per sample, add_message out, no flush ever), driven
    as capt_sched.c drives it: a consumer that wakes every 50 ms and hands on what has arrived (receiver/capt_sched.c:484-528),
    at 252 kS/s of wall clock (tests/harness/shim_realtime.c).  The library books the latency of every frame itself
    (nvx_shim_latency: entry of the sample_in_1 call of the frame's last sample -> bits pollable, messages at add_message):
    below 100 ms throughout; and the message reaches add_message within 100 ms of the call that completed its frame."""
    text = "ZCZC RT42\nREAL TIME 5678\nNNNN\n"
    st, _ = signals.stream_params(nv, 778, nv.RATE_IN, n_phasing=12, text=text)
    n_frames = 26
    iq = nv.synth_host(st, nv.RATE_IN, n_frames * nv.FRAME_IN)
    ref = oracle.Pipe(chain_mask=3, charlayer=True)
    k_done = None
    for k in range(n_frames):
        ref.push(iq[k * nv.FRAME_IN:(k + 1) * nv.FRAME_IN])
        if ref.messages:
            k_done = k + 1; break
    assert k_done is not None and ref.messages[0][:2] == (518, "RT42")
    data = tmp_path / "iq.bin"; iq.tofile(data)
    exe = tmp_path / "shim_realtime"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O2", str(ROOT / "tests" / "harness" / "shim_realtime.c"), "-o", str(exe), f"-L{lib}", "-lnavtex_amd",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe), str(data)], check=True, capture_output=True, text=True, timeout=120).stdout
    fed = {int(l.split()[1]): float(l.split()[2]) for l in out.splitlines() if l.startswith("FED ")}
    msgs = [(float(l.split()[1]), l.split()[2]) for l in out.splitlines() if l.startswith("MSG ")]
    lat = next(l.split() for l in out.splitlines() if l.startswith("LAT "))
    frames, p50, p99, worst = int(lat[1]), float(lat[2]), float(lat[3]), float(lat[4])
    assert len(fed) == n_frames and frames >= n_frames - 1, out[-600:]
    assert 0 < p50 <= p99 <= worst < 100.0, lat
    assert msgs and msgs[0][1] == "518|RT42", msgs
    delay = msgs[0][0] - fed[k_done - 1]
    assert -1.0 <= delay <= 100.0, f"the message arrived {delay:.1f} ms after the call that completed its frame (frame {k_done})"


@pytest.mark.gpu
def test_stream_callback_on_a_handle_of_its_own_delivers_within_a_callback_interval(nv, oracle):
    """the SDRplay callback shape on a push-mode handle -- no ring, no poller, the vendor thread is
    the only caller (receiver/capt_sched.c:105-148 does its work in the callback too).  Every push takes in what has finished
    meanwhile, so the message is at the sink a few callbacks after its frame was complete -- not a frame later, with the
    next launch."""
    from fake_sdr import FakeSdr
    text = "ZCZC CB09\nCALLBACK ONLY 42\nNNNN\n"
    st, _ = signals.stream_params(nv, 779, nv.RATE_IN, n_phasing=12, text=text)
    n_frames = 26
    iq = nv.synth_host(st, nv.RATE_IN, n_frames * nv.FRAME_IN)
    ref = oracle.Pipe(chain_mask=1, charlayer=True)
    k_done = None
    for k in range(n_frames):
        ref.push(iq[k * nv.FRAME_IN:(k + 1) * nv.FRAME_IN])
        if ref.messages:
            k_done = k + 1; break
    assert k_done is not None

    with nv.Pipeline(n_streams=1, raw_rate=False, chain_mask=nv.CHAIN_518, max_frames=2, push_mode=True, char_layer=True) as p:
        arrived = []
        class Vendor:                                           # the vendor library's streaming thread calls this
            def feed(self, xi, xq):
                nv.lib.nvx_StreamACallback(xi.ctypes.data, xq.ctypes.data, None, xi.shape[0], 0, p._h)
                if p.messages and not arrived:
                    arrived.append(time.monotonic())
        sdr = FakeSdr(Vendor(), iq, nv.RATE_IN, nv.FRAME_IN, seed=11, packet=(150, 420))
        sdr.start(); sdr.join()
        assert arrived and p.messages[0][1:] == ref.messages[0] and sdr.late_ms < 50.0
        delay_ms = (arrived[0] - sdr.frame_done_at[k_done - 1]) * 1e3
        assert 0.0 <= delay_ms <= 50.0, f"message {delay_ms:.1f} ms after its frame was complete"
        p.flush()
        want = oracle.Pipe(chain_mask=1, charlayer=False); want.push(iq)
        assert p.bits(0, 0) == want.bits(0)
