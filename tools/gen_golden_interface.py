#!/usr/bin/env python3
"""Golden record of how the REAL reference's own code uses its `dsp` module (tests/golden/reference_dsp_interface.json),
so that tests/test_option_a_module_swap.py checks INTEGRATION.md option A without a reference checkout.  The reference is
imported, never copied; what goes into the fixture is data:

* every `dsp.<name>` the reference's modules take from the module, and every `<x>.demodulator.<attr>` they read;
* the PacketConfig call protocol.Parser makes when it is constructed (protocol.py:68-76, 115-116), recorded through a
  stand-in `rtldavis.dsp` that forwards to the reference's real dsp module;
* the public attributes of the reference's PacketConfig for that call, and the arrays its Demodulator holds;
* the error its demodulate() raises for an input of the wrong size.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_interface.py <reference checkout>/src
"""
import ast
import glob
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True


def encode(v):
    if isinstance(v, np.ndarray):
        return {"ndarray": v.dtype.str, "values": v.tolist()}
    if isinstance(v, bytes):
        return {"bytes": v.hex()}
    return v


def names_used(src_dir):
    """dsp.<name> and <x>.demodulator.<attr> over the reference's modules (dsp.py itself excluded)."""
    dsp_names, dem_attrs = set(), set()
    for path in sorted(glob.glob(os.path.join(src_dir, "rtldavis", "**", "*.py"), recursive=True)):
        if os.path.basename(path) == "dsp.py":
            continue
        with open(path) as fh:
            tree = ast.parse(fh.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "dsp":
                dsp_names.add(node.attr)
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Attribute) and node.value.attr == "demodulator":
                dem_attrs.add(node.attr)
    return sorted(dsp_names), sorted(dem_attrs)


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.environ["RTLDAVIS_REFERENCE"]
    sys.path.insert(0, src)
    import rtldavis  # noqa: F401  (the package itself)
    real = importlib.import_module("rtldavis.dsp")

    calls = []
    proxy = types.ModuleType("rtldavis.dsp")

    def recording_packet_config(*args, **kwargs):
        calls.append({"args": list(args), "kwargs": kwargs})
        return real.PacketConfig(*args, **kwargs)

    for k, v in vars(real).items():
        setattr(proxy, k, v)
    proxy.PacketConfig = recording_packet_config
    sys.modules["rtldavis.dsp"] = proxy
    rtldavis.dsp = proxy
    protocol = importlib.import_module("rtldavis.protocol")
    parser = protocol.Parser(symbol_length=14)
    assert len(calls) == 1 and type(parser.demodulator) is real.Demodulator
    assert parser.parse([]) == []

    cfg = real.PacketConfig(*calls[0]["args"], **calls[0]["kwargs"])
    dem = real.Demodulator(cfg)
    arrays = {k: {"shape": list(v.shape), "dtype": v.dtype.str} for k, v in vars(dem).items() if isinstance(v, np.ndarray)}
    try:
        dem.demodulate(np.zeros(10, np.uint8))
        raise AssertionError("the reference accepted a 10-byte block")
    except ValueError as e:
        size_error = str(e)
    dsp_names, dem_attrs = names_used(src)
    out = {
        "generator": "tools/gen_golden_interface.py",
        "dsp_names_used": dsp_names,
        "demodulator_attrs_used": dem_attrs,
        "parser_packet_config_call": {"symbol_length": 14, **calls[0]},
        "packet_config": {k: encode(v) for k, v in sorted(vars(cfg).items())},
        "demodulator_arrays": arrays,
        "size_error": {"type": "ValueError", "message": size_error},
    }
    with open(os.path.join(ROOT, "tests", "golden", "reference_dsp_interface.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
