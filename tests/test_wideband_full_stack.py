"""A WidebandReceiver with every per-chunk feature switched on at once, on the device: per-channel gain, retune, levels,
spectrum, the device-side parse, burst detection with per-chunk thresholds, burst decode with repair behind the
narrow-band filter, expected-slot decode and burst quality, at the two configurations of tests/full_stack_cases.py
(3 channels "s16" and 70 channels "u8").  The gains, thresholds, the expectation table and the tuning change between
the same two submits with two chunks in flight; every accessor is read after each fetch with the next chunk already
submitted and compared with full_stack_cases.compose(), which puts the suite's existing models together: the channelized
bytes against the float64 model and its a-priori bound, everything else - on the receiver's own bytes - exactly.  Then
the same run one chunk at a time, every feature group alone, a reset in the middle, the switches taken off in the order
of their dependencies, and the last rows of every slot at 70 channels and 64 expectations.  tests/test_full_stack_cpu.py
shows on the model alone that these inputs reach what they are meant to reach."""
import functools

import numpy as np
import pytest

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_quality_cases as QC
import burst_track_cases as TK
import chan_bound as CB
import full_stack_cases as FS
import gain_cases as GC
import retune_cases as RC
import spectrum_model as SM
from stream_parse_helpers import _pkey, _rows, assert_rows_match
from rtldavis_amd.wideband import BURST_THRESHOLD_OFF, QUALITY_DTYPE

pytestmark = pytest.mark.gpu

FRONT = ("levels", "spectrum", "parsed")
CHAIN = ("bursts", "messages", "expected", "quality_m", "quality_x")
EVERYTHING = FRONT + CHAIN
TUNING = ("set_gain", "retune")                              # what the plain and the front twin take of the schedule
READ = dict(levels="levels", spectrum="spectrum", parsed="parsed", bursts="bursts", messages="burst_messages",
            expected="expected_messages", quality_m="burst_message_quality", quality_x="expected_message_quality")


def _device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"


@functools.lru_cache(maxsize=None)
def _thr0(name):
    """Thresholds from the floor of a chunk of noise alone, received at the first gains."""
    _device()
    cfg = FS.config(name)
    rx = FS.receiver(cfg)
    rx.set_gain(cfg.gains[0])
    rx.set_bursts(True)
    rx.demodulate(cfg.quiet)
    return FS.thresholds_of(cfg, rx.bursts().floor)


def _schedule(name):
    return FS.actions(FS.config(name), _thr0(name))


def _only(sched, methods):
    return {k: [(m, a) for m, a in acts if m in methods] for k, acts in sched.items()}


def _switch_on(rx, cfg, parts):
    if parts == EVERYTHING:
        FS.switch_on(rx, cfg)
    elif parts == FRONT:
        rx.set_levels(True)
        rx.set_spectrum(cfg.n_bins)
        rx.set_parse(True)
    elif parts == CHAIN:
        rx.set_bursts(True)
        rx.set_burst_decode(True)
        rx.set_burst_repair(FS.MAX_FLIPS)
        rx.set_burst_narrow(FS.NARROW)
        rx.set_burst_quality(True, cfg.gap)
    else:
        assert parts == ()


def _take(rx, packets, parts, chunk):
    """What the last fetch left: the channelized bytes, the packets, the capture chunk and every accessor of ``parts``."""
    out = dict(block=rx.channelized(), packets=_pkey(packets), chunk=chunk)
    for p in parts:
        out[p] = getattr(rx, READ[p])()
    return out


def _stream(rx, sched, chunks, parts, in_flight=True, first=0, seen=None):
    """submit, submit, [actions], fetch, submit, ... (or one chunk at a time): the actions of chunk k are applied before its
    submit - with chunks k - 2 and k - 1 in flight -, every accessor is read after a fetch with the next chunk submitted."""
    got, fed = [], []

    def take():
        got.append(_take(rx, rx.fetch(), parts, fed[len(got)]))

    for k, chunk in enumerate(chunks, first):
        if k in sched:
            assert rx.inflight == (min(k - first, 2) if in_flight else 0)
            FS.apply(rx, sched[k])
        if seen is not None:
            seen.append((rx.gains(), rx.burst_thresholds(), rx.burst_expect(), rx.tuning()))
        fed.append(chunk)
        if in_flight:
            if k - first >= 2:
                take()                                      # chunk k - 2; chunk k - 1 in flight
            rx.submit(chunk)
        else:
            got.append(_take(rx, rx.demodulate(chunk), parts, chunk))
    while in_flight and len(got) < len(fed):
        take()
    return got


def _run(name, parts=EVERYTHING, in_flight=True, methods=None):
    _device()
    cfg = FS.config(name)
    sched = _schedule(name)
    rx = FS.receiver(cfg)
    _switch_on(rx, cfg, parts)
    seen = []
    got = _stream(rx, sched if methods is None else _only(sched, methods), cfg.chunks, parts, in_flight, seen=seen)
    return got, seen, rx


@functools.lru_cache(maxsize=None)
def _all_on(name):
    return _run(name)


@functools.lru_cache(maxsize=None)
def _composed(name):
    return FS.compose(FS.config(name), _all_on(name)[0], _schedule(name))


def _same(a, b, parts, what):
    """Two takes hold the same bytes: every record array, every header field."""
    assert a["block"].tobytes() == b["block"].tobytes(), (what, "channelized")
    assert a["packets"] == b["packets"], (what, "packets")
    for p in parts:
        x, y = a[p], b[p]
        if p == "levels":
            assert x.channels.tobytes() == y.channels.tobytes() and tuple(x.input) == tuple(y.input) and x.chunk == y.chunk, (what, p)
        elif p == "spectrum":
            assert x.power.tobytes() == y.power.tobytes() and x.segments == y.segments and x.chunk == y.chunk, (what, p)
        elif p == "bursts":
            assert x.records.tobytes() == y.records.tobytes() and x.floor.tobytes() == y.floor.tobytes() and x.chunk == y.chunk, (what, p)
        elif p == "messages":
            assert x.records.tobytes() == y.records.tobytes() and x.long_runs.tobytes() == y.long_runs.tobytes() and x.chunk == y.chunk, (what, p)
        elif p == "expected":
            assert x.records.tobytes() == y.records.tobytes() and x.candidates.tobytes() == y.candidates.tobytes() and x.chunk == y.chunk, (what, p)
        else:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, p)


def _assert_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got, want)
    for f in got.dtype.names:
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def _assert_front(cfg, k, g, w, what):
    have = [(int(r["peak"]), int(r["clipped"]), int(r["power"])) for r in g["levels"].channels]
    assert g["levels"].chunk == k and have == w["levels"][0], (what, k, "levels")
    assert g["levels"].channels["gain"].dtype == np.float32 and g["levels"].channels["gain"].tolist() == w["levels"][1].tolist(), (what, k)
    assert tuple(g["levels"].input) == w["levels"][2], (what, k, "input level")
    sp, (p, s, _) = g["spectrum"], w["spectrum"]
    assert sp.power.shape == (cfg.n_bins,) and sp.segments == s and sp.chunk == k, (what, k, "spectrum")
    assert np.array_equal(sp.freqs_hz, SM.freqs(RC.CENTRE, cfg.fw, cfg.n_bins))
    ratio = SM.excess(sp.power, p, cfg.n_bins)                # per bin: spectrum_model.tol_bin
    assert ratio <= 1.0, (what, k, "spectrum", ratio)
    assert_rows_match(_rows(g["parsed"]), w["parsed"], (what, k, "parsed"))
    return ratio


def _assert_chain(cfg, k, g, w, what, quality=True):
    BC.assert_equals_model(g["bursts"], g["block"], w["thr"], k)
    DC.assert_equals_model(g["messages"], w["messages"])
    x = g["expected"]
    assert x.chunk == k and np.array_equal(x.candidates, w["expected"].candidates), (what, k, x.candidates, w["expected"].candidates)
    _assert_records(x.records, w["expected"].records, (what, k, "expected"))
    if quality:
        for j, p in enumerate(("quality_m", "quality_x")):
            assert g[p].dtype == QUALITY_DTYPE and g[p].shape == (g["messages"].records, x.records)[j].shape
            _assert_records(g[p], w["quality"][j], (what, k, p))


def _as_composed(got):
    """A device run in the shape of compose()'s result, for full_stack_cases.counts."""
    return [dict(messages=g["messages"], expected=g["expected"], quality=(g["quality_m"], g["quality_x"]),
                 parsed=[(r, None) for r in _rows(g["parsed"])]) for g in got]


@pytest.mark.parametrize("name", FS.NAMES)
def test_every_accessor_equals_its_model(name):
    cfg = FS.config(name)
    got, seen, _ = _all_on(name)
    want = _composed(name)
    force = FS.in_force(cfg, _schedule(name))
    assert len(got) == cfg.nk == len(want)
    for k, (g, t, x, (shift, phase)) in enumerate(seen):      # what each submit saw: every change holds from the next submit
        f = force[k]
        assert g.tolist() == f["gains"].tolist() and t.tolist() == f["thr"].tolist() and x.tobytes() == f["table"].tobytes(), k
        assert (tuple(int(v) for v in shift), tuple(int(v) for v in phase)) == f["tuning"], k
    for k, (g, w) in enumerate(zip(got, want)):
        rows, Z, delta = w["channelized"]
        s = CB.check_against_model(g["block"][rows], Z, delta)
        ratio = _assert_front(cfg, k, g, w, name)
        _assert_chain(cfg, k, g, w, name)
        print(f"\n[full-stack] {name} chunk {k}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{g['block'][rows].size}, "
              f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta); spectrum err / tol_bin {ratio:.4f}; records: "
              f"parsed {len(g['parsed'])} bursts {g['bursts'].records.size} messages {g['messages'].records.size} "
              f"expected {g['expected'].records.size} quality {g['quality_m'].size}+{g['quality_x'].size} "
              f"packets {sum(len(p) for p in g['packets'])}")
        assert s["bad_lsb"] == 0 and s["bad_exact"] == 0, (k, s)
        assert s["exempt"] <= GC.GPU_EXEMPT_CAP, (k, s)
    c = FS.counts(cfg, got, _as_composed(got))
    print(f"\n[full-stack] {name}: {c}")
    assert c["messages"] >= 3 and len(c["message_channels"]) >= 2 and c["expected"] >= 3, c
    assert name != "wide" or (0 in c["message_channels"] and 69 in c["message_channels"]), c
    assert c["repaired"] >= 1 and c["lookback_after_retune"] >= 1 and c["dropped"] >= 1, c
    assert c["quality_rows"] == c["messages"] + c["expected"] == c["inband"] and c["with_noise"] >= 1, c
    assert c["parsed"] >= 1 and c["in_both"] >= 1, c


@pytest.mark.parametrize("name", FS.NAMES)
def test_in_flight_equals_one_at_a_time(name):
    cfg = FS.config(name)
    flight, _, _ = _all_on(name)
    quiet, _, rx = _run(name, in_flight=False)
    for k, (a, b) in enumerate(zip(flight, quiet)):
        _same(a, b, EVERYTHING, (name, k))
    # two more chunks - the capture's last two again, their expectations moved along with the clock - at another noise gap
    assert rx.inflight == 0
    rx.set_burst_quality(True, cfg.other_gap)
    tab = FS.tables(cfg)[2].copy()
    tab["t_lo"] += 2 * FS.BS
    tab["t_hi"] += 2 * FS.BS
    sched = dict(_schedule(name))
    sched[cfg.nk] = [("set_burst_expect", tab)]
    more = _stream(rx, sched, cfg.chunks[-2:], EVERYTHING, in_flight=False, first=cfg.nk)
    want = FS.compose(cfg, quiet + more, sched, gaps=[cfg.gap] * cfg.nk + [cfg.other_gap] * 2, channel_model=False)
    rows = moved = 0
    for k in (cfg.nk, cfg.nk + 1):
        g, w = more[k - cfg.nk], want[k]
        _assert_front(cfg, k, g, w, name)
        _assert_chain(cfg, k, g, w, name)
        prev = (quiet + more)[k - 1]["block"]
        for recs, q in ((g["messages"].records, g["quality_m"]), (g["expected"].records, g["quality_x"])):
            rows += q.size
            moved += int((QC.quality_rows(g["block"], prev, cfg.cfg, recs, cfg.gap, k)["noise"] != q["noise"]).sum())
    assert rows >= 2 and moved >= 1, (rows, moved)           # the new gap shows: the old one gives another noise sum


@pytest.mark.parametrize("name", FS.NAMES)
def test_each_feature_alone_gives_the_same_records(name):
    every, _, _ = _all_on(name)
    plain, _, _ = _run(name, (), methods=TUNING)
    front, _, _ = _run(name, FRONT, methods=TUNING)
    chain, _, _ = _run(name, CHAIN)
    for k, a in enumerate(every):
        _same(a, plain[k], (), (name, k, "plain"))
        _same(a, front[k], FRONT, (name, k, "front"))
        _same(a, chain[k], CHAIN, (name, k, "chain"))


@pytest.mark.parametrize("name", FS.NAMES)
def test_reset_in_the_middle_reproduces_the_run(name):
    _device()
    cfg = FS.config(name)
    sched = _schedule(name)
    first, _, _ = _all_on(name)
    rx = FS.receiver(cfg)
    FS.switch_on(rx, cfg)
    FS.apply(rx, sched[0])
    rx.submit(cfg.chunks[0])
    rx.submit(cfg.chunks[1])
    for k in (2, 3):
        FS.apply(rx, sched.get(k, ()))
        rx.fetch()
        rx.submit(cfg.chunks[k])
    rx.fetch()
    assert rx.inflight == 1 and rx.burst_messages().chunk == 2
    rx.set_gain(cfg.gains[2][::-1].copy())                   # pending at the reset: a gain, a retune and a table
    rx.retune(-cfg.retune)
    rx.set_burst_expect(FS.tables(cfg)[0])
    rx.reset()
    assert rx.inflight == 0 and rx.gains().tolist() == [cfg.gain] * cfg.n_ch
    assert rx.burst_thresholds().tolist() == [BURST_THRESHOLD_OFF] * cfg.n_ch and rx.burst_expect().size == 0
    assert [int(v) for v in rx.tuning()[0]] == [int(v) for v in cfg.plan_shift] and not np.any(rx.tuning()[1])
    assert rx.burst_repair() == FS.MAX_FLIPS and rx.burst_narrow() is FS.NARROW and rx.burst_quality() == (True, cfg.gap)

    def nothing_yet():
        for fn in [rx.channelized] + [getattr(rx, READ[p]) for p in EVERYTHING]:
            with pytest.raises(RuntimeError):
                fn()

    nothing_yet()
    FS.apply(rx, sched[0])                                   # what a reset drops: gains, thresholds, the table
    rx.submit(cfg.chunks[0])
    nothing_yet()                                            # submitted, not fetched
    rx.submit(cfg.chunks[1])
    FS.apply(rx, sched[2])
    again = [_take(rx, rx.fetch(), EVERYTHING, cfg.chunks[0])]
    rx.submit(cfg.chunks[2])
    again += [_take(rx, rx.fetch(), EVERYTHING, cfg.chunks[k]) for k in (1, 2)]
    for k in range(3):
        _same(first[k], again[k], EVERYTHING, (name, k))
    assert sum(a["messages"].records.size + a["expected"].records.size for a in again) >= 2


@pytest.mark.parametrize("name", FS.NAMES)
def test_switching_off_in_dependency_order(name):
    cfg = FS.config(name)
    sched = _schedule(name)
    run, _, rx = _run(name)
    force = FS.in_force(cfg, sched)[-1]
    rx.set_burst_decode(False)
    pk = rx.demodulate(cfg.chunks[0])
    off = dict(block=rx.channelized(), packets=_pkey(pk), chunk=cfg.chunks[0])
    for p in FRONT + ("bursts",):
        off[p] = getattr(rx, READ[p])()
    want = FS.compose(cfg, run + [dict(off, bursts=off["bursts"])], sched, channel_model=False)[cfg.nk]
    _assert_front(cfg, cfg.nk, off, want, name)
    BC.assert_equals_model(off["bursts"], off["block"], force["thr"], cfg.nk)
    for p in ("messages", "expected", "quality_m", "quality_x"):
        with pytest.raises(RuntimeError):
            getattr(rx, READ[p])()
    assert rx.burst_repair() == 0 and rx.burst_narrow() is False and rx.burst_quality()[0] is False and rx.burst_expect().size == 0
    # decode and quality back on, the narrow-band filter not: the quality kernel needs the filter's table, the decoder none
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    rx.set_burst_quality(True)
    assert rx.burst_narrow() is False and rx.burst_quality() == (True, 0)
    k = cfg.nk + 1
    planted = cfg.chunks[-1]                                  # (a burst lies wholly inside the capture's last chunk)
    rx.demodulate(planted)
    block, bursts, m, x = rx.channelized(), rx.bursts(), rx.burst_messages(), rx.expected_messages()
    qm, qx = rx.burst_message_quality(), rx.expected_message_quality()
    BC.assert_equals_model(bursts, block, force["thr"], k)
    model = NB.decode_model(block, off["block"], bursts, cfg.cfg, True, k * FS.BS, 0, narrow=False)
    DC.assert_equals_model(m, model)                          # (the chunk before delivered no message: nothing to drop)
    assert m.records.size >= 1 and not (m.records["flags"] & NB.NARROW).any()
    assert x.records.size == 0 and x.candidates.size == 0 and qx.size == 0
    _assert_records(qm, QC.quality_rows(block, off["block"], cfg.cfg, m.records, 0, k), (name, "quality without narrow"))
    assert np.all(qm["flags"] == QC.INBAND)


def _full_table(cfg):
    """RD_BX_MAX rows: 62 on channels spread over the plan - windows in every chunk, noise alone in most -, then the last
    burst of channel 0 and, as row 63, the weak burst of channel 69 (in chunk 3, tuned as from the retune on)."""
    rows = []
    for i in range(TK.MAX - 2):
        t = (i % cfg.nk) * FS.BS + 200 + 23 * i
        rows.append(TK.expect_row((11 * i) % cfg.n_ch, t, t + 40, TK.corr_of(FS.IF_HZ / FS.FO)))
    tab = TK.table(rows)
    last = FS.expect_table(cfg, [cfg.planted[-1], next(p for p in cfg.planted if p[0] == 69 and p[2] >= 3 * FS.BS)], True, extra=False)
    return np.concatenate([tab, last])


def test_rows_of_the_last_channel_and_the_last_expectation():
    name = "wide"
    _device()
    cfg = FS.config(name)
    tab = _full_table(cfg)
    assert tab.size == TK.MAX and int(tab[-1]["channel"]) == cfg.n_ch - 1 == 69
    sched = {k: [(m, tab if m == "set_burst_expect" else a) for m, a in acts] for k, acts in _schedule(name).items()}
    rx = FS.receiver(cfg)
    FS.switch_on(rx, cfg)
    got = _stream(rx, sched, cfg.chunks, EVERYTHING)
    want = FS.compose(cfg, got, sched, channel_model=False)
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_chain(cfg, k, g, w, name)
        assert g["expected"].candidates.size == TK.MAX
    g = got[3]
    assert g["messages"].records.size >= 1 and int(g["messages"].records[-1]["channel"]) == 69     # the message slot's last channel
    assert g["quality_m"].size == g["messages"].records.size and int(g["quality_m"][-1]["flags"]) == QC.INBAND
    x = g["expected"].records
    assert x.size >= 1 and int(x[-1]["first"]) == TK.MAX - 1 and int(x[-1]["channel"]) == 69       # expectation 63
    assert bytes(x[-1]["data"]) == bytes(FS.weak_packet()) and int(g["quality_x"][-1]["flags"]) == QC.INBAND
    assert sum(int((a["expected"].candidates > 0).sum()) for a in got) >= TK.MAX // 2              # the rows were searched
