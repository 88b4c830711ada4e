"""The band scan (include/navtex_amd_scan.h) on the GPU (-m gpu): power rows bit-identical to the restatement
(tests/scan_ref.py) for every input kind, in both kernel forms, at the rails and on silence; the host entry; 1024
streams with a carrier each; and the product path scan -> nvx_set_carrier -> decode -> signal report."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import scan_ref as sr
import signals

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KINDS = [(True, 1), (True, 3), (False, 1)]
KIND_IDS = ["raw", "raw-cic3", "252k"]


@pytest.fixture(scope="module")
def sc(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_scan.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.scan
    yield navtex_amd.scan
    navtex_amd.scan.set_form(0)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _frame(nv, raw):
    return nv.FRAME_RAW if raw else nv.FRAME_IN


def _iq(nv, raw, frames, sid, freq_hz=14000, amplitude=8000, text=None):
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    st, _ = signals.stream_params(nv, sid, rate, freq_hz=freq_hz, amplitude=amplitude, text=text)
    return nv.synth_host(st, rate, frames * _frame(nv, raw))


def _upload(nv, iqs, pitch):
    buf = nv.DeviceBuffer(len(iqs) * pitch * 4)
    for s, iq in enumerate(iqs):
        buf.upload(iq, s * pitch * 4)
    return buf


@pytest.mark.parametrize("form", [1, 2], ids=["per-stream", "per-frame+fold"])
@pytest.mark.parametrize("raw,s0", KINDS, ids=KIND_IDS)
def test_rows_are_bit_identical_to_the_restatement(nv, sc, raw, s0, form):
    """Several different streams in one call, a pitch larger than the data, one frame and several, first_frame > 0."""
    frames = 3
    iqs = [_iq(nv, raw, frames, 40 + s, f) for s, f in enumerate((14000, -5003, 1000))]
    pitch = frames * _frame(nv, raw) + 4096
    buf = _upload(nv, iqs, pitch)
    y1 = [sr.front(iq, raw, s0) for iq in iqs]
    sc.set_form(form)
    for f0, nf in ((0, 1), (0, 3), (1, 2), (2, 1)):
        got = sc.scan_resident(buf, pitch, f0, nf, len(iqs), raw, s0)
        for s in range(len(iqs)):
            assert np.array_equal(_u64(got[s]), _u64(sr.power_row(y1[s], f0, nf))), (f0, nf, s)
    buf.free()


@pytest.mark.parametrize("raw,s0", KINDS, ids=KIND_IDS)
def test_rails_and_silence_in_both_forms(nv, sc, raw, s0):
    """Full-scale random input, both rails held and alternating, and silence: identical in both forms and to the restatement."""
    n = 2 * _frame(nv, raw)
    rng = np.random.default_rng(17)
    rails = np.empty((n, 2), dtype=np.int16)
    rails[:, 0] = np.where((np.arange(n) // 5) % 2, 32767, -32768)
    rails[:, 1] = -32768
    iqs = [rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16), rails, np.full((n, 2), 32767, dtype=np.int16), np.zeros((n, 2), dtype=np.int16)]
    buf = _upload(nv, iqs, n)
    want = [sr.power_row(sr.front(iq, raw, s0), 0, 2) for iq in iqs]
    assert not want[3].any()
    rows = {}
    for form in (1, 2):
        sc.set_form(form)
        rows[form] = sc.scan_resident(buf, n, 0, 2, len(iqs), raw, s0)
        for s in range(len(iqs)):
            assert np.array_equal(_u64(rows[form][s]), _u64(want[s])), (form, s)
    assert np.array_equal(_u64(rows[1]), _u64(rows[2]))
    buf.free()


def test_the_default_form_follows_the_shape_and_both_are_launched(nv, sc):
    """Below 512 streams the frames are spread over workgroups (two launches of the timing's count stay one call); from
    512 on a workgroup walks a stream.  Same rows either way."""
    raw, frames, n = False, 2, 520
    iq = _iq(nv, raw, frames, 77, 3000)
    pitch = frames * nv.FRAME_IN
    buf = _upload(nv, [iq] * n, pitch)
    want = sr.power_row(sr.front(iq, raw), 0, frames)
    sc.set_form(0)
    launches = sc.debug_last_launch()["launches"]
    big = sc.scan_resident(buf, pitch, 0, frames, n, raw)
    last = sc.debug_last_launch()
    assert last["form"] == 1 and last["grid"] == (n, 1) and last["scratch_bytes"] == 0 and last["launches"] == launches + 1, last
    small = sc.scan_resident(buf, pitch, 0, frames, 7, raw)
    last = sc.debug_last_launch()
    assert last["form"] == 2 and last["grid"] == (frames, 7) and last["scratch_bytes"] == 7 * frames * sc.FFT * 8 and last["launches"] == launches + 2, last
    assert all(np.array_equal(_u64(big[s]), _u64(want)) for s in range(n))
    assert all(np.array_equal(_u64(small[s]), _u64(want)) for s in range(7))
    buf.free()


@pytest.mark.parametrize("raw,s0", KINDS, ids=KIND_IDS)
def test_host_entry_gives_the_resident_row_and_ignores_a_partial_frame(nv, sc, raw, s0):
    frames = 2
    iq = _iq(nv, raw, frames + 1, 60, -9000)[:frames * _frame(nv, raw) + 12345]
    row, used = sc.scan_iq(iq, raw, s0)
    assert used == frames
    buf = _upload(nv, [iq[:frames * _frame(nv, raw)]], frames * _frame(nv, raw))
    res = sc.scan_resident(buf, frames * _frame(nv, raw), 0, frames, 1, raw, s0)[0]
    buf.free()
    assert np.array_equal(_u64(row), _u64(res)) and np.array_equal(_u64(row), _u64(sr.scan(iq, raw, s0, 0, frames)))


def test_scale_1024_raw_streams_a_random_carrier_each(nv, sc):
    n, frames = 1024, 2
    rng = np.random.default_rng(23)
    freqs = rng.integers(-24000, 24001, size=n)
    streams = [signals.stream_params(nv, 2000 + s, nv.RATE_RAW, freq_hz=int(freqs[s]))[0] for s in range(n)]
    pitch = frames * nv.FRAME_RAW
    buf = nv.DeviceBuffer(n * pitch * 4)
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    sc.set_form(0)
    rows = sc.scan_resident(buf, pitch, 0, frames, n, True, 1)
    buf.free()
    worst = 0.0
    for s in range(n):
        hits = sc.find(rows[s])
        assert hits, s
        worst = max(worst, abs(hits[0]["offset_hz"] - freqs[s]))
        assert abs(hits[0]["offset_hz"] - freqs[s]) <= 5.0, (s, int(freqs[s]), hits[:2])
    print("worst strongest-hit error over", n, "streams:", round(worst, 2), "Hz")

    def want(s):
        return sr.scan(nv.synth_host(streams[s], nv.RATE_RAW, pitch), True, 1)
    spread = list(range(0, n, 32))
    with ThreadPoolExecutor(16) as ex:
        for s, w in zip(spread, ex.map(want, spread)):
            assert np.array_equal(_u64(rows[s]), _u64(w)), s


CARRIERS = ((150.0, "ZCZC AA01\nCARRIER PLUS 150 HZ\nNNNN\n"), (1000.0, "ZCZC AB02\nCARRIER PLUS 1 KHZ\nNNNN\n"),
            (-5000.0, "ZCZC AC03\nCARRIER MINUS 5 KHZ\nNNNN\n"), (19000.0, "ZCZC AD04\nCARRIER PLUS 19 KHZ\nNNNN\n"))


def test_the_product_path_scan_tune_decode_report(nv, sc):
    """A handle that does not know where its streams' carriers are: the scan says, nvx_set_carrier goes there, the
    messages arrive, and the signal reports see the carriers within 10 Hz of where the chains were tuned."""
    frames = 40
    iqs = [_iq(nv, False, frames, 700 + i, int(hz), text=txt) for i, (hz, txt) in enumerate(CARRIERS)]
    pitch = frames * nv.FRAME_IN
    buf = _upload(nv, iqs, pitch)
    rows = sc.scan_resident(buf, pitch, 0, 3, len(iqs), False)
    buf.free()
    with nv.Pipeline(n_streams=len(CARRIERS), chain_mask=nv.CHAIN_518, max_frames=4, push_mode=True) as p:
        p.enable_signal_report(True)
        for s, (hz, _) in enumerate(CARRIERS):
            hits = sc.find(rows[s])
            assert len(hits) == 1 and abs(hits[0]["offset_hz"] - hz) <= 5.0, (s, hits)
            applied = p.set_carrier(s, 0, hits[0]["offset_hz"])
            assert abs(applied - hz) <= 5.0 + 3.125 / 2
        for s in range(len(CARRIERS)):
            p.push(s, iqs[s])
        p.flush()
        got = {s: [m[3] for m in p.messages if m[0] == s] for s in range(len(CARRIERS))}
        reports = [p.signal_report(s, 0) for s in range(len(CARRIERS))]
    for s, (_, txt) in enumerate(CARRIERS):
        assert got[s] == [txt], (s, got[s])
        print(s, "report offset", round(reports[s]["offset_hz"], 2), "shift", round(reports[s]["shift_hz"], 1))
        assert abs(reports[s]["offset_hz"]) <= 10.0, (s, reports[s])


def test_errors_and_timing(nv, sc):
    ARG = nv._native.ERR_ARG
    frames = 2
    iq = _iq(nv, False, frames, 5)
    pitch = frames * nv.FRAME_IN
    buf = _upload(nv, [iq, iq], pitch)
    out = nv.DeviceBuffer(2 * sc.FFT * 8)
    small = nv.DeviceBuffer(sc.FFT * 8)
    call = lambda *a: sc.lib.nvx_scan_resident(0, *a)            # noqa: E731
    ok = (buf.ptr, pitch, 0, frames, 2, 0, 1, out.ptr, None)
    assert call(*ok) == 0 and nv.lib.nvx_device_sync(0) == 0
    bad = {"three frames of two": (buf.ptr, pitch, 0, 3, 2, 0, 1, out.ptr, None),
           "first frame beyond the data": (buf.ptr, pitch, 2, 1, 2, 0, 1, out.ptr, None),
           "a third stream": (buf.ptr, pitch, 0, frames, 3, 0, 1, out.ptr, None),
           "raw frames in a 252 kS/s buffer": (buf.ptr, pitch, 0, 1, 2, 1, 1, out.ptr, None),
           "rows for one stream": (buf.ptr, pitch, 0, frames, 2, 0, 1, small.ptr, None),
           "stage 0 at 252 kS/s": (buf.ptr, pitch, 0, frames, 2, 0, 3, out.ptr, None),
           "pitch not a multiple of 4": (buf.ptr, pitch + 2, 0, 1, 1, 0, 1, out.ptr, None),
           "misaligned input": (buf.ptr + 4, pitch, 0, 1, 1, 0, 1, out.ptr, None),
           "no device 99": None}
    for name, args in bad.items():
        rc = sc.lib.nvx_scan_resident(99, *ok) if args is None else call(*args)
        assert rc == ARG, (name, rc)
        assert sc.lib.nvx_scan_last_error() != b""
    with pytest.raises(nv.NvxError) as e:
        sc.scan_iq(iq[:1000], False)
    assert e.value.code == ARG
    # timing: one count per call, whichever form
    sc.timing(True)
    sc.time_stats(reset=True)
    for form in (1, 2, 1):
        sc.set_form(form)
        assert call(*ok) == 0
    ms, n = sc.time_stats()
    assert n == 3 and ms > 0.0
    sc.timing(False)
    assert call(*ok) == 0
    assert sc.time_stats(reset=True)[1] == 3 and sc.time_stats() == (0.0, 0)
    for b in (buf, out, small):
        b.free()
