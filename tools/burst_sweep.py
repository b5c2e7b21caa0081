#!/usr/bin/env python3
"""The seeded sweep of the burst kernels (tests/burst_sweep_cases.py) over any range of seeds, for hunting beyond the
suite's fixed SEEDS by hand.  Not run by the suite.

Without --device every chain of the range is built on the models alone: the conditions the case modules assert on their
own models run, the counts of burst_sweep_cases.tally are summed and printed, and the first seed whose chain fails to
build is named.  With --device every family of every chain also goes through its test hook - the launching and
comparing code of tests/test_burst_sweep.py - and the first seed and family whose slot differs from the model's is
printed with the difference.  Needs a device then; there is no fall-back.  Exit status 1 when a seed was named.

    python tools/burst_sweep.py 352 2000              # models alone
    python tools/burst_sweep.py 352 2000 --device     # against the MI355X
    python -c "import burst_sweep_cases as S; S.chain(SEED)"     (in tests/) rebuilds a named seed
"""
import argparse
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_sweep_cases as S  # noqa: E402


def on_device(lib, T, ch):
    """Every family of one chain on the device; raises AssertionError naming the launch that differs."""
    sc = ch.scene
    T.T_BURSTS._assert_bursts(ch.bursts, *T._bursts(lib, sc, ch.bursts))
    T._assert_decode(ch.decode, T._decode(lib, sc, ch.decode))
    T._assert_expect(ch.expect, T._expect(lib, sc, ch.expect))
    if ch.search is not None:
        T.T_SEARCH._assert_slot(ch.search, T._search(lib, sc, ch.search))
    T.T_QUALITY._assert_slot(ch.quality, T._quality(lib, sc, ch.quality))
    T.T_CLIPS._assert_slot(ch.clips, T._clips(lib, sc, ch.clips))
    if ch.replay is not None:
        T._assert_replay(ch.replay, T._replay(lib, sc, ch.replay))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("first", type=int, help="the first seed")
    ap.add_argument("last", type=int, help="one past the last seed")
    ap.add_argument("--device", action="store_true", help="compare every slot with the device's")
    args = ap.parse_args()
    lib = T = None
    if args.device:
        import test_burst_sweep as T
        lib = T._lib_with_device()
    total, slots = Counter(), 0
    for seed in range(args.first, args.last):
        try:
            ch = S.chain(seed)
            total.update(S.tally(ch))
            if args.device:
                on_device(lib, T, ch)
        except AssertionError as e:
            print(f"seed {seed}: {'the device differs from the model' if args.device else 'the chain does not build'}: {e}")
            return 1
        slots += sum(getattr(ch, f) is not None for f in S.FAMILIES)
    print(f"seeds {args.first} .. {args.last - 1}: {slots} launches built{' and equal on the device' if args.device else ''}")
    for k in sorted(total, key=str):
        print(f"    {k}: {total[k]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
