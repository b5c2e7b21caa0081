"""The inputs of tests/test_wideband_full_stack.py do what tests/full_stack_cases.py says they do - checked here, on the
float64 model alone: the bytes are the channelizer oracle's (model_z + quantise) under the schedule of gains, retunes,
thresholds and tables, the burst records the model's, and compose() says what a receiver with everything switched on
must deliver for them.  Every test is a condition on the inputs: enough records by either decoder, on the first and
the last channel, a repaired one, a look-back right after the retune, a record step 7 drops together with its quality
row, quality rows with a noise window, a packet parsed() and burst_messages() both hold, few bytes near a rounding
boundary, and a schedule that asks for nothing a receiver with chunks in flight refuses."""
import functools

import numpy as np
import pytest

import burst_quality_cases as QC
import burst_repair_cases as RP
import chan_bound as CB
import full_stack_cases as FS
import gain_cases as GC


@functools.lru_cache(maxsize=None)
def _model(name):
    cfg = FS.config(name)
    run, sched = FS.model_run(cfg)
    want = FS.compose(cfg, run, sched)
    c = FS.counts(cfg, run, want)
    print(f"\n[full-stack model] {name}: {c}")
    return cfg, run, sched, want, c


@pytest.mark.parametrize("name", FS.NAMES)
def test_burst_messages_on_several_channels(name):
    cfg, _, _, _, c = _model(name)
    assert c["messages"] >= 3 and len(c["message_channels"]) >= 2, c
    if name == "wide":
        assert 0 in c["message_channels"] and cfg.n_ch - 1 == 69 in c["message_channels"], c


@pytest.mark.parametrize("name", FS.NAMES)
def test_expected_messages_and_the_rows_that_find_nothing(name):
    cfg, _, sched, want, c = _model(name)
    assert c["expected"] >= 3, c
    force = FS.in_force(cfg, sched)
    searched = 0
    for k, w in enumerate(want):
        n = force[k]["table"].size
        x = w["expected"]
        assert x.candidates.size == n and n >= 3              # (past the table's end the slot says RD_BX_NO_ENTRY)
        idle, nothing = n - 2, n - 1                          # the table's last two rows
        assert x.candidates[idle] == 0
        assert not np.isin(x.records["first"], (idle, nothing)).any()
        searched += int(x.candidates[nothing] > 0)
    assert searched >= 1                                      # the row where no burst is was searched, and found nothing


@pytest.mark.parametrize("name", FS.NAMES)
def test_a_repaired_record(name):
    _, _, _, want, c = _model(name)
    assert c["repaired"] >= 1, c
    rows = [r for w in want for r in w["messages"].records if int(r["flags"]) & RP.REPAIRED]
    assert any(bytes(r["data"]) == bytes(FS.weak_packet()) and list(r["pad"][:3]) == [2, 41, 66] for r in rows)


@pytest.mark.parametrize("name", FS.NAMES)
def test_a_look_back_right_after_the_retune(name):
    cfg, _, sched, _, c = _model(name)
    assert any(m == "retune" for m, _ in sched[cfg.retune_at])
    assert c["lookback_after_retune"] >= 1, c


@pytest.mark.parametrize("name", FS.NAMES)
def test_step_7_drops_a_record_and_its_quality_row(name):
    cfg, run, _, want, c = _model(name)
    assert c["dropped"] >= 1, c
    plain = FS.undropped(cfg, run)
    for k, (p, w) in enumerate(zip(plain, want)):
        kept = w["messages"].records
        assert w["quality"][0].shape == kept.shape            # rows parallel to what is delivered
        if p.records.size > kept.size:
            gone = [r for r in p.records if r.tobytes() not in {q.tobytes() for q in kept}]
            assert gone and all(int(r["flags"]) & 1 and int(r["tau"]) < 0 for r in gone), k
            before = [q for q in want[k - 1]["messages"].records if bytes(q["data"]) == bytes(gone[0]["data"])]
            assert before and abs(int(before[0]["time"]) - int(gone[0]["time"])) < FS.SL


@pytest.mark.parametrize("name", FS.NAMES)
def test_quality_rows_are_inband_and_have_a_noise_window(name):
    _, _, _, _, c = _model(name)
    assert c["quality_rows"] == c["messages"] + c["expected"] and c["inband"] == c["quality_rows"], c
    assert c["with_noise"] >= 1, c


@pytest.mark.parametrize("name", FS.NAMES)
def test_a_packet_in_parsed_and_in_burst_messages(name):
    _, _, _, _, c = _model(name)
    assert c["parsed"] >= 1 and c["in_both"] >= 1, c


@pytest.mark.parametrize("name", FS.NAMES)
def test_few_bytes_of_the_model_lie_near_a_rounding_boundary(name):
    cfg, run, _, want, _ = _model(name)
    shares = []
    for k, w in enumerate(want):
        rows, Z, delta = w["channelized"]
        s = CB.check_against_model(run[k]["block"][rows], Z, delta)
        assert s["mismatches"] == 0                           # (the bytes are this model's)
        shares.append(s["exempt"])
    print(f"\n[full-stack model] {name}: exempt share per chunk {' '.join(f'{s:.2%}' for s in shares)}")
    assert max(shares) <= GC.MODEL_EXEMPT_CAP, shares


@pytest.mark.parametrize("name", FS.NAMES)
def test_the_schedule_asks_for_nothing_that_needs_a_quiet_receiver(name):
    cfg, _, sched, _, _ = _model(name)
    assert sorted(sched) == [0, 2, cfg.retune_at] and 2 < cfg.retune_at < cfg.nk - 1
    for k, acts in sched.items():
        assert not [m for m, _ in acts if m in FS.SWITCHES_NEED_QUIET], k
    assert [m for m, _ in sched[2]] == ["set_gain", "set_burst_threshold", "set_burst_expect"]
    assert [m for m, _ in sched[cfg.retune_at]][:2] == ["retune", "set_gain"]
    g = cfg.gains
    assert np.array_equal(g[0] != g[2], cfg.subset) and np.all(g[2] != g[cfg.retune_at]) and len(set(g[0].tolist())) >= 3
    assert np.all(cfg.retune != 0) and 0 < cfg.gap != cfg.other_gap <= QC.MAX_GAP
