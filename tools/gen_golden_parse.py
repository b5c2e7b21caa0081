#!/usr/bin/env python3
"""Generate tests/golden/parse_gate.json by running the REAL reference parser (build container only) on the
production-config cases of tests/parse_gate_cases.py: for every packet of every call its index and bytes, the verdict of
the reference's own swap_bit_order + CRC.checksum(data[2:]), the id and the protocol.py:304-311 frequency error on the
real demodulator's discriminated buffer, and whether Parser.parse returned a message for it.  The Parser is built as
the reference builds it; for block sizes other than its own 8192 its cfg and demodulator are replaced by the
reference's PacketConfig / Demodulator of that block size before the first block.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_parse.py

Everything written is data (burst specification, recorded results); no reference source.
"""
from __future__ import annotations

import hashlib
import json
import logging
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RTLDAVIS_REFERENCE", "/root/reference/src")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rtldavis import dsp as ref_dsp  # noqa: E402  (the real reference)
from rtldavis import protocol as ref_protocol  # noqa: E402
import parse_gate_cases as PG  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "parse_gate.json")


def run_case(B: int) -> dict:
    case = PG.prod_case(B)
    parser = ref_protocol.Parser(symbol_length=14)
    if parser.cfg.block_size != B:
        c = parser.cfg
        parser.cfg = ref_dsp.PacketConfig(c.bit_rate, c.symbol_length, c.preamble_symbols, c.packet_symbols, c.preamble, B)
        parser.demodulator = ref_dsp.Demodulator(parser.cfg)
    cfg, dem = parser.cfg, parser.demodulator
    calls = []
    for blk in case.blocks():
        pk = dem.demodulate(blk)
        msgs = parser.parse(pk)
        got = {id(m.packet) for m in msgs}
        rec = []
        for p in pk:
            data = bytes(ref_protocol.swap_bit_order(b) for b in p.data)
            mean = np.mean(dem.discriminated[p.index: p.index + cfg.preamble_length])
            fe = -int((mean * float(cfg.sample_rate)) / (2 * math.pi))
            rec.append({"index": int(p.index), "data": bytes(p.data).hex(),
                        "crc_ok": bool(parser._crc.checksum(data[2:]) == 0), "id": int(data[2] & 7), "freq_err": int(fe),
                        "message": id(p) in got})
        calls.append(rec)
    return {"block_size": B, "n_blocks": case.n_blocks, "seed": case.seed,
            "bursts": [{"data": bytes(o).hex(), "start": int(s), "cfo": float(c)} for o, s, c in case.bursts],
            "raw_sha256": hashlib.sha256(case.raw.tobytes()).hexdigest(), "calls": calls}


def main() -> None:
    logging.disable(logging.CRITICAL)
    out = {"generator": "tools/gen_golden_parse.py", "numpy": np.__version__,
           "cases": {str(B): run_case(B) for B in PG.PROD_BLOCK_SIZES}}
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    n = sum(len(c) for g in out["cases"].values() for c in g["calls"])
    m = sum(p["message"] for g in out["cases"].values() for c in g["calls"] for p in c)
    print(f"{OUT}: {n} packets, {m} messages from the real parser")


if __name__ == "__main__":
    main()
