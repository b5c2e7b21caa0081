"""INTEGRATION.md option A: the reference's own protocol.Parser running on rtldavis_amd.dsp through a
module swap.  CPU only - constructing the Parser / Demodulator must not touch the GPU (the parent
process builds one before it forks the worker, runners/rtlsdr.py:30, __main__.py:277).  What the reference's
code takes from its dsp module is pinned as data in tests/golden/reference_dsp_interface.json
(tools/gen_golden_interface.py, run against the real reference): the names it uses, the PacketConfig call
Parser.__post_init__ makes (protocol.py:68-76, 115-116), its PacketConfig's attributes and its Demodulator's arrays."""
import types

import numpy as np
import pytest

from conftest import load_json


@pytest.fixture(scope="module")
def iface():
    return load_json("reference_dsp_interface.json")


def decode(v):
    if isinstance(v, dict) and "ndarray" in v:
        return np.array(v["values"], dtype=np.dtype(v["ndarray"]))
    if isinstance(v, dict) and "bytes" in v:
        return bytes.fromhex(v["bytes"])
    return v


def assert_same_attr(got, want, name):
    if isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), name
    else:
        assert type(got) is type(want) and got == want, name


def test_reference_parser_builds_on_the_hip_dsp_without_a_gpu(iface):
    import rtldavis_amd.dsp as hip_dsp
    for name in iface["dsp_names_used"]:  # everything the reference's modules take from `dsp`
        assert hasattr(hip_dsp, name), f"dsp.{name}"
    call = iface["parser_packet_config_call"]  # what Parser(symbol_length=14) passes, then dsp.Demodulator(cfg)
    assert call["symbol_length"] == 14
    cfg = hip_dsp.PacketConfig(*call["args"], **call["kwargs"])
    dem = hip_dsp.Demodulator(cfg)
    assert type(dem) is hip_dsp.Demodulator and type(cfg) is hip_dsp.PacketConfig and dem.cfg is cfg
    for name, want in iface["packet_config"].items():
        assert_same_attr(getattr(cfg, name), decode(want), name)
    c = cfg
    assert (c.bit_rate, c.symbol_length, c.block_size, c.preamble_length, c.buffer_length) == (19200, 14, 8192, 224, 16384)
    for name in iface["demodulator_attrs_used"]:  # what protocol.Parser reads from its demodulator
        assert hasattr(dem, name), f"demodulator.{name}"
    from rtldavis_amd import _lib
    assert _lib.lib().rd_demod_inflight(dem._h) == 0
    # size errors are the reference's (dsp.py:145-149) and come before any device work
    err = iface["size_error"]
    assert err["type"] == "ValueError"
    with pytest.raises(ValueError, match=err["message"]):
        dem.demodulate(np.zeros(10, np.uint8))


def test_demodulator_accepts_the_references_packet_config(iface):
    """A PacketConfig of the reference's (here: an object with exactly its attributes) is accepted as is."""
    import rtldavis_amd.dsp as hip_dsp
    ref_cfg = types.SimpleNamespace(**{k: decode(v) for k, v in iface["packet_config"].items()})
    dem = hip_dsp.Demodulator(ref_cfg)  # host state only
    assert dem.cfg is ref_cfg
    for name in ("quantized", "discriminated", "filtered"):  # the reference's arrays, zeros before the first call
        want = iface["demodulator_arrays"][name]
        got = getattr(dem, name)
        assert got.shape == tuple(want["shape"]) and got.dtype == np.dtype(want["dtype"]) and not got.any(), name
