"""Wideband front-end (build-owned): the 8-channel polyphase
channeliser.  CPU: the scalar restatement against an ideal float filter bank.
GPU: the HIP kernel bit-exact against the restatement, and a wideband stream with
16 NAVTEX carriers decoded end to end."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

FS = 2016000


def tone(freq, n, amp=8000.0):
    t = np.arange(n)
    x = amp * np.exp(2j * np.pi * freq * t / FS)
    return np.stack([np.round(x.real), np.round(x.imag)], 1).astype(np.int16)


def ideal_filterbank(raw, taps_q18):
    """float64 reference: mix each sub-band to DC, FIR with the same taps, decimate by 8
    (newest sample of output m is 8m+7)."""
    x = raw[:, 0].astype(np.float64) + 1j * raw[:, 1].astype(np.float64)
    h = np.asarray(taps_q18, dtype=np.float64) / (1 << 18)
    n = np.arange(x.size)
    out = []
    for k in range(8):
        y = np.convolve(x * np.exp(-2j * np.pi * k * n / 8), h)[: x.size]
        out.append(y[7::8])
    return np.array(out)


def taps():
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "navtex_amd" / "csrc" / "nvx_pfb_taps.h").read_text()
    body = src[src.index("NVX_PFB_H[48]"):]
    return [int(v) for v in re.findall(r"-?\d+", body[body.index("{"): body.index("}")])]


def test_taps_are_shared_and_sane():
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    a = (root / "navtex_amd" / "csrc" / "nvx_pfb_taps.h").read_text().split("{")[1]
    b = (root / "oracle" / "nvx_oracle_pfb_taps.h").read_text().split("{")[1]
    assert a == b
    h = taps()
    assert len(h) == 48 and sum(h) == 1 << 18 and h == h[::-1] and max(map(abs, h)) < 32768


def test_restatement_is_a_filter_bank(oracle):
    rng = np.random.default_rng(4)
    n = 8 * 3000
    raw = (tone(14000, n, 3000).astype(np.int32) + tone(252000 - 14000, n, 2500) + tone(-3 * 252000 + 5000, n, 2000)
           + rng.integers(-1500, 1501, size=(n, 2))).astype(np.int16)
    got = oracle.channelise(raw).astype(np.float64)
    got = got[:, :, 0] + 1j * got[:, :, 1]
    want = ideal_filterbank(raw, taps())
    err = np.abs(got - want)[:, 8:]                      # skip the start-up of the FIR
    assert err.max() < 3.0                                # integer rounding only (a few LSB of 2^15)
    power = (np.abs(got[:, 100:]) ** 2).mean(axis=1)
    assert np.argsort(power)[-3:].tolist().sort() == [0, 1, 5].sort()


def test_restatement_history_chaining(oracle):
    rng = np.random.default_rng(5)
    raw = rng.integers(-32768, 32768, size=(8 * 640, 2), dtype=np.int16)
    whole = oracle.channelise(raw)
    a = oracle.channelise(raw[: 8 * 256])
    b = oracle.channelise(raw[8 * 256:], hist40=raw[8 * 256 - 40: 8 * 256])
    assert np.array_equal(whole, np.concatenate([a, b], axis=1))


@pytest.mark.gpu
def test_kernel_bit_exact_full_scale_random(nv, oracle):
    rng = np.random.default_rng(6)
    n_wide, n_out = 3, 64 * 40
    raw = rng.integers(-32768, 32768, size=(n_wide, 8 * n_out, 2), dtype=np.int16)
    raw[0, :4000] = 32767; raw[1, :4000] = -32768           # saturating stretches -> clamp path
    pitch_raw, pitch_sub = 8 * n_out + 8, n_out + 4
    d_raw = nv.DeviceBuffer(n_wide * pitch_raw * 4); d_sub = nv.DeviceBuffer(n_wide * 8 * pitch_sub * 4)
    h0, h1 = nv.DeviceBuffer(n_wide * 40 * 4), nv.DeviceBuffer(n_wide * 40 * 4)
    for w in range(n_wide):
        d_raw.upload(raw[w], offset=w * pitch_raw * 4)
    first = 64 * 24
    # two calls with carried history == one call == the restatement
    nv.channelise(d_raw, pitch_raw, 0, n_wide, first, d_sub, pitch_sub, 0, hist_in=None, hist_out=h0)
    nv.channelise(d_raw, pitch_raw, 8 * first, n_wide, n_out - first, d_sub, pitch_sub, first, hist_in=h0, hist_out=h1)
    got = d_sub.download(n_wide * 8 * pitch_sub * 4, dtype=np.int16).reshape(n_wide * 8, pitch_sub, 2)[:, :n_out]
    for w in range(n_wide):
        want = oracle.channelise(raw[w])
        assert np.array_equal(got[8 * w: 8 * w + 8], want), f"wide stream {w}"
    assert np.array_equal(h1.download(n_wide * 40 * 4, dtype=np.int16).reshape(n_wide, 40, 2), raw[:, -40:])
    for b in (d_raw, d_sub, h0, h1):
        b.free()


@pytest.mark.gpu
def test_sixteen_carriers_from_one_wideband_stream(nv, oracle):
    """One 2.016 MS/s stream with a NAVTEX carrier at k*252 kHz +-14 kHz for every k: the
    channeliser + the 252 kS/s pipeline decode all 16 messages, bits identical to the
    restatement chain (channeliser restatement -> oracle pipeline)."""
    n_frames = 36                                       # 11.5 s: phasing (2.8 s) + ~45 characters twice (6.3 s) + priming
    n = n_frames * nv.FRAME_RAW
    total = np.zeros((n, 2), dtype=np.int32)
    texts = {}
    for k in range(8):
        centre = k * 252000 if k < 4 else (k - 8) * 252000
        carriers = []
        for c, off in ((0, 14000), (1, -14000)):
            txt = f"ZCZC W{chr(65 + k)}{k}{c}\nBAND {k} CHAIN {c}\nNNNN\n"
            texts[(k, c)] = txt
            carriers.append(dict(freq_hz=centre + off, bits=nv.sitor_encode(txt, 20), bit_offset=(977 * (2 * k + c + 1)) % 20160,
                                 phase0=(123456789 * (2 * k + c + 1)) % 2**32, amplitude=1700))
        total += nv.synth_host(nv.make_stream(carriers, seed=k, noise_amp=0), nv.RATE_RAW, n)
    rng = np.random.default_rng(0)
    total += rng.integers(-600, 601, size=total.shape)
    raw = np.clip(total, -32768, 32767).astype(np.int16)

    n_out = n // 8
    d_raw = nv.DeviceBuffer(n * 4); d_sub = nv.DeviceBuffer(8 * n_out * 4)
    d_raw.upload(raw)
    nv.channelise(d_raw, n, 0, 1, n_out, d_sub, n_out)
    sub = oracle.channelise(raw)
    assert np.array_equal(d_sub.download(8 * n_out * 4, dtype=np.int16).reshape(8, n_out, 2), sub)

    labels = [[1000 * (k + 1) + 518, 1000 * (k + 1) + 490] for k in range(8)]
    with nv.Pipeline(n_streams=8, raw_rate=False, chain_mask=3, labels=labels, max_frames=n_frames) as p:
        p.process_resident(d_sub, n_out, 0, n_frames)
        p.fetch()
        got = {(s, f % 1000): (b, m) for (s, f, b, m) in p.messages}
        for k in range(8):
            ref = oracle.Pipe(chain_mask=3, charlayer=False)
            ref.push(sub[k])
            for c, f in ((0, 518), (1, 490)):
                assert p.bits(k, c) == ref.bits(c), f"band {k} chain {c}"
                assert got[(k, f)] == (f"W{chr(65 + k)}{k}{c}", texts[(k, c)]), f"band {k} chain {c}"
    # the same through the wideband handle mode: three launches (history ping-pong, channeliser of
    # launch k+1 overlapping the cascade of launch k), then once more through the host-fed push path
    wl = [[1000 * (k + 1) + 518, 1000 * (k + 1) + 490] for k in range(8)]
    with nv.Pipeline(n_streams=1, wideband=True, chain_mask=3, labels=wl, max_frames=12) as p:
        for f0 in (0, 12, 24):
            p.process_resident(d_raw, n, f0, 12)
        p.fetch()
        msgs = {(s, f % 1000): (b, m) for (s, f, b, m) in p.messages}
        for k in range(8):
            ref = oracle.Pipe(chain_mask=3, charlayer=False)
            ref.push(sub[k])
            for c, f in ((0, 518), (1, 490)):
                assert p.bits(k, c) == ref.bits(c), f"wideband handle: band {k} chain {c}"
                assert msgs[(k, f)] == (f"W{chr(65 + k)}{k}{c}", texts[(k, c)])
        resident_bits = [p.bits(k, c) for k in range(8) for c in (0, 1)]
    with nv.Pipeline(n_streams=1, wideband=True, chain_mask=3, labels=wl, max_frames=5, push_mode=True, char_layer=False) as p:
        rng = np.random.default_rng(2)
        pos = 0
        while pos < n:
            m = int(min(n - pos, rng.integers(1000, 3 * nv.FRAME_RAW)))
            p.push(0, raw[pos:pos + m]); pos += m
        p.flush()
        assert [p.bits(k, c) for k in range(8) for c in (0, 1)] == resident_bits
    d_raw.free(); d_sub.free()


@pytest.mark.gpu
def test_fused_wideband_kernel_against_the_restatement_chain(nv, oracle, tmp_path):
    """The fused wideband kernel (a wideband handle's kernel) on several streams x several frames per launch, so that
    units of one stream hand their histories over between workgroups: the 900 S/s output of all 16 chains of every
    stream is bit-identical to channeliser restatement -> oracle cascade, bits too; masks select chains.  (Run in a
    process of its own: the digest of everything it produced travels back as one JSON line.)"""
    import hashlib, os, subprocess, sys
    script = tmp_path / "wb.py"
    script.write_text('''
import sys, hashlib, json
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, navtex_amd as nv
W, F = 5, 7
n = F * nv.FRAME_RAW
rng = np.random.default_rng(11)
raw = np.empty((W, n, 2), dtype=np.int16)
for w in range(W):
    carriers = []
    for k in range(8):
        centre = k * 252000 if k < 4 else (k - 8) * 252000
        for c, off in ((0, 14000), (1, -14000)):
            carriers.append(dict(freq_hz=centre + off, bits=nv.sitor_encode(f"ZCZC AA{(w + k + c) % 100:02d}\\nW{w} K{k} C{c}\\nNNNN\\n", 6),
                                 bit_offset=(911 * (16 * w + 2 * k + c + 1)) % 20160, phase0=(7654321 * (16 * w + 2 * k + c + 1)) % 2**32, amplitude=1500))
    raw[w] = nv.synth_host(nv.make_stream(carriers, seed=40 + w, noise_amp=500), nv.RATE_RAW, n)
masks = [(3, 1, 2, 3, 3, 2, 1, 3)[(i + i // 8) % 8] for i in range(8 * W)]
buf = nv.DeviceBuffer(W * n * 4)
buf.upload(raw)
h = hashlib.sha256()
out = {}
with nv.Pipeline(n_streams=W, wideband=True, chain_masks=masks, max_frames=4, char_layer=False) as p:
    for f0, k in ((0, 4), (4, 3)):
        p.process_resident(buf, n, f0, k); p.fetch()
        for s in range(8 * W):
            for c in range(2):
                if (masks[s] >> c) & 1:
                    y = p.debug_y3(s, c); h.update(y.tobytes())
                    out.setdefault(f"{s}.{c}", []).append(y.tobytes().hex() if s in (0, 13, 39) else "")
    bits = {f"{s}.{c}": p.bits(s, c) for s in range(8 * W) for c in range(2)}
    for k in sorted(bits): h.update(bits[k].encode())
np.save(sys.argv[2], raw)
print(json.dumps({"digest": h.hexdigest(), "bits": bits, "masks": masks, "y3": {k: v for k, v in out.items() if v[0]}}))
''')
    root = str(Path(__file__).resolve().parent.parent)
    r = subprocess.run([sys.executable, str(script), root, str(tmp_path / "raw.npy")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    raw = np.load(tmp_path / "raw.npy")
    W, masks = raw.shape[0], rec["masks"]
    for w in range(W):
        sub = oracle.channelise(raw[w])
        for k in range(8):
            s = 8 * w + k
            ref = oracle.Pipe(chain_mask=masks[s], charlayer=False, tap_y3=7 * nv.FRAME_Y3)
            ref.push(sub[k])
            for c in range(2):
                want = ref.bits(c) if (masks[s] >> c) & 1 else ""
                assert rec["bits"][f"{s}.{c}"] == want, f"wide {w} band {k} chain {c}"
                if f"{s}.{c}" in rec["y3"]:
                    got = np.frombuffer(bytes.fromhex("".join(rec["y3"][f"{s}.{c}"])), dtype=np.float64).reshape(-1, 2)
                    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(ref.y3(c)).view(np.uint64)), f"y3 of stream {s} chain {c}"


@pytest.mark.gpu
def test_fused_kernel_unit_hand_over_chain(nv, oracle):
    """Two wideband streams x 20 frames in ONE launch: every (stream, frame) unit gets its own workgroup and each stream is
    a 20-deep chain of hand-overs (filter histories of 8 sub-bands x 2 chains and the channeliser's 40-sample halo) between
    workgroups that all spin at once.  The complete 900 S/s output of every chain must be bit-exact against the
    restatement chain; three rounds (L1-warm consumers on the later ones), then split into launches of 7 + 13 frames."""
    W, F = 3, 20
    n = F * nv.FRAME_RAW
    rng = np.random.default_rng(21)
    raw = rng.integers(-9000, 9000, size=(W, n, 2), dtype=np.int16)           # wideband noise: every sub-band busy
    # third stream: full-scale random with saturating stretches (constant +-full scale, full-scale tones at sub-band
    # centres): the output clamp of the channeliser and the largest intermediate values of its transform
    raw[2] = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    raw[2, 5000:60000] = 32767; raw[2, 90000:140000] = -32768
    t = np.arange(200000)
    for k, at in ((1, 300000), (3, 600000), (6, 900000)):
        ph = 2 * np.pi * k * t / 8.0 + 0.3
        raw[2, at:at + t.size, 0] = np.clip(np.round(32767.0 * np.cos(ph)), -32768, 32767).astype(np.int16)
        raw[2, at:at + t.size, 1] = np.clip(np.round(32767.0 * np.sin(ph)), -32768, 32767).astype(np.int16)
    for w in range(2):
        car = [dict(freq_hz=(k * 252000 if k < 4 else (k - 8) * 252000) + off, bits=nv.sitor_encode(f"ZCZC HO{k}{c}\nX\nNNNN\n", 8),
                    bit_offset=1000 * k + 77 * c + 13 * w + 1, phase0=k * 999 + c, amplitude=1200) for k in range(8) for c, off in ((0, 14000), (1, -14000))]
        raw[w] = np.clip(raw[w].astype(np.int32) + nv.synth_host(nv.make_stream(car, seed=5 + w, noise_amp=0), nv.RATE_RAW, n), -32768, 32767).astype(np.int16)
    want = {}
    for w in range(W):
        sub = oracle.channelise(raw[w])
        for k in range(8):
            ref = oracle.Pipe(chain_mask=3, charlayer=False, tap_y3=F * nv.FRAME_Y3)
            ref.push(sub[k])
            for c in range(2):
                want[(8 * w + k, c)] = (np.ascontiguousarray(ref.y3(c)).view(np.uint64).copy(), ref.bits(c))
    buf = nv.DeviceBuffer(W * n * 4)
    buf.upload(raw)
    with nv.Pipeline(n_streams=W, wideband=True, chain_mask=3, max_frames=F, char_layer=False) as p:
        for rep, plan in enumerate(([F], [F], [F], [7, 13])):
            p.reset()
            got = {key: [] for key in want}
            f0 = 0
            for k in plan:
                p.process_resident(buf, n, f0, k); f0 += k
                p.fetch()
                for (s, c) in want:
                    got[(s, c)].append(p.debug_y3(s, c)[: k * nv.FRAME_Y3].copy())
            for (s, c), (y3, bits) in want.items():
                assert np.array_equal(np.concatenate(got[(s, c)]).view(np.uint64), y3), f"round {rep}: stream {s} chain {c}"
                assert p.bits(s, c) == bits
    buf.free()


def _fused_units_run(nv, independent):
    W, F = 1, 48
    n = F * nv.FRAME_RAW
    car = [dict(freq_hz=(k * 252000 if k < 4 else (k - 8) * 252000) + off, bits=nv.sitor_encode(f"ZCZC IU{k}{c}\nREPLAY\nNNNN\n", 10),
                bit_offset=1000 * k + 77 * c + 1, phase0=k * 999 + c, amplitude=1500) for k in range(8) for c, off in ((0, 14000), (1, -14000))]
    buf = nv.DeviceBuffer(W * n * 4)
    nv.synth_device([nv.make_stream(car, seed=9, noise_amp=700)], nv.RATE_RAW, n, buf, n)
    h = hashlib.sha256()
    with nv.Pipeline(n_streams=W, wideband=True, chain_mask=3, max_frames=29, char_layer=False, forms=(independent, -1, -1)) as p:
        p.process_resident(buf, n, 0, 29); p.fetch()                  # warm-up + first half
        assert p.last_forms()[:2] == (independent, -1)
        for s in range(8):
            for c in range(2): h.update(p.debug_y3(s, c).tobytes())
        p.process_resident(buf, n, 29, 19); p.fetch()
        assert p.last_forms()[:2] == (independent, -1)
        for s in range(8):
            for c in range(2):
                h.update(p.debug_y3(s, c).tobytes()); h.update(p.bits(s, c).encode())
        nbits = sum(len(p.bits(s, c)) for s in range(8) for c in range(2))
        p.reset(); p.enable_timing(True); p.kernel_time_stats(0, reset=True)
        for _ in range(3):
            p.process_resident(buf, n, 0, 29)
        p.fetch()
        assert p.last_forms()[:2] == (independent, -1)
        ms, k = p.kernel_time_stats(0)
    buf.free()
    return {"digest": h.hexdigest(), "kernel_ms": ms / k, "bits": nbits}


@pytest.mark.gpu
def test_fused_dependent_and_independent_units_agree_bit_for_bit(nv):
    """The fused wideband kernel's two unit forms (r3): hand-over from frame to frame (many streams) and independent units
    that pre-roll nine passes with the real channeliser halo in front (few streams -- ONE RSP capture replayed from a
    recording is the physically real case, receiver/capt_sched.c:356-417).  Forced either way: the
    900 S/s output and the bits of a 29-frame + 19-frame pair of launches of ONE wideband stream are identical, and the
    independent form is what makes that workload use more than one CU (>= 10 x faster; measured ~40 x)."""
    recs = [_fused_units_run(nv, independent) for independent in (0, 1)]
    assert recs[0]["digest"] == recs[1]["digest"] and recs[0]["bits"] > 16 * 1000
    print(f"one wideband stream x 29 frames: hand-over {recs[0]['kernel_ms']:.2f} ms, independent units {recs[1]['kernel_ms']:.2f} ms")
    assert recs[1]["kernel_ms"] * 10 < recs[0]["kernel_ms"]


@pytest.mark.gpu
def test_group_of_wideband_handles(nv, oracle):
    """Wideband inputs sharded over group members: 3 wideband streams over 2 members (2 + 1), masks and labels per decoded
    stream (8 per input), global ids in the messages."""
    W, F = 3, 30
    n = F * nv.FRAME_RAW
    raw = np.empty((W, n, 2), dtype=np.int16)
    texts = {}
    for w in range(W):
        car = []
        for k in range(8):
            centre = k * 252000 if k < 4 else (k - 8) * 252000
            txt = f"ZCZC G{chr(65 + w)}{k:02d}\nW{w} B{k}\nNNNN\n"
            texts[8 * w + k] = txt
            car.append(dict(freq_hz=centre + 14000, bits=nv.sitor_encode(txt, 14), bit_offset=(1234 * (8 * w + k + 1)) % 20160, phase0=w * 77 + k, amplitude=2500))
        raw[w] = nv.synth_host(nv.make_stream(car, seed=70 + w, noise_amp=800), nv.RATE_RAW, n)
    masks = [1] * (8 * W)
    labels = [[5000 + i, 0] for i in range(8 * W)]
    bufs = [nv.DeviceBuffer(2 * n * 4), nv.DeviceBuffer(1 * n * 4)]
    bufs[0].upload(raw[:2]); bufs[1].upload(raw[2:])
    import ctypes as C
    from navtex_amd import _native as N          # through the C ABI directly: the Python Group wrapper has no wideband switch
    cfg = N.Config(); nv.lib.nvx_config_default(C.byref(cfg))
    cfg.n_streams, cfg.wideband, cfg.max_frames, cfg.char_layer = W, 1, 10, 1
    m_arr = (C.c_uint8 * len(masks))(*masks); cfg.chain_masks = m_arr
    l_arr = (C.c_int * (2 * len(labels)))(*[v for pair in labels for v in pair]); cfg.labels = l_arr
    msgs = []
    cb = N.MESSAGE_FN(lambda u, s, b, m, f: msgs.append((s, f, b.decode(), m.decode()))); cfg.on_message = cb
    devs = (C.c_int * 2)(0, 0)
    g = C.c_void_p()
    N.check(nv.lib.nvx_group_create(devs, 2, C.byref(cfg), C.byref(g)), "nvx_group_create")
    try:
        ptrs = (C.c_void_p * 2)(bufs[0].ptr, bufs[1].ptr)
        for f0 in (0, 10, 20):
            N.check(nv.lib.nvx_group_process_resident(g, ptrs, n, f0, 10), "process")
        N.check(nv.lib.nvx_group_fetch_bits(g), "fetch")
        # members own INPUT streams (2 + 1); decoded stream ids stay 8 * w + k with w the GLOBAL input stream
        assert nv.lib.nvx_group_member_of(g, 0) == 0 and nv.lib.nvx_group_member_of(g, 1) == 0 and nv.lib.nvx_group_member_of(g, 2) == 1
        assert msgs == sorted(msgs, key=lambda t: t[0])               # delivered member after member, stream after stream
        assert [(s, f, b, m) for (s, f, b, m) in msgs] == [(i, 5000 + i, f"G{chr(65 + i // 8)}{i % 8:02d}", texts[i]) for i in range(8 * W)]
        out = C.create_string_buffer(1 << 16)
        for w in range(W):
            sub = oracle.channelise(raw[w])
            for k in (0, 5):
                ref = oracle.Pipe(chain_mask=1, charlayer=False); ref.push(sub[k])
                nb = nv.lib.nvx_group_poll_bits(g, 8 * w + k, 0, out, 1 << 16)
                assert out.raw[:nb].decode() == ref.bits(0) and nv.lib.nvx_group_bit_count(g, 8 * w + k, 0) == nb
    finally:
        nv.lib.nvx_group_destroy(g)
    for b in bufs:
        b.free()


@pytest.mark.gpu
def test_wideband_full_size_total_parity(nv, oracle):
    """The wideband bench workload at full size (512 streams x 2.016 MS/s x 12 frames = 15.9 GB, 8192 carriers): EVERY
    carrier's bits from the fused kernel equal the restatement chain's (oracle channeliser -> 8 x two-chain oracle
    pipelines, OpenMP over the wideband streams), and no bit-timing decision is near a tie."""
    import os, sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import bench, signals
    W, F = 512, 12
    n = F * nv.FRAME_RAW
    try:
        buf = nv.DeviceBuffer(W * n * 4)
    except nv.NvxError:
        pytest.skip("not enough device memory")
    nv.synth_device(bench.wideband_streams(nv, signals, 0, W), nv.RATE_RAW, n, buf, n)
    ncpu = min(16, len(os.sched_getaffinity(0)))
    with nv.Pipeline(n_streams=W, wideband=True, chain_mask=3, max_frames=F, char_layer=False) as p:
        p.process_resident(buf, n, 0, F)
        p.fetch()
        bad, chunk = [], 32
        for w0 in range(0, W, chunk):
            sample = buf.download(chunk * n * 4, offset=w0 * n * 4, dtype=np.int16).reshape(chunk, n, 2)
            _secs, want = oracle.bench_wide(sample, chunk, n // 8, ncpu, want_bits=True)
            for i, bits in enumerate(want):
                s, c = 8 * w0 + i // 2, i % 2
                if p.bits(s, c) != bits or len(bits) < 300:
                    bad.append((s, c))
        near, evals, margin = p.tie_stats()
    buf.free()
    assert bad == [], f"{len(bad)} of {16 * W} carriers differ: {bad[:10]}"
    assert near == 0 and evals > 16 * W * 250
