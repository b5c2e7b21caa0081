"""CPU-side checks: the C-ABI library loads and exports every symbol the header declares,
argument errors surface as the reference's exceptions, and no compute happens without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from rtldavis_amd import _lib
    L = _lib.lib()
    names = header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/rtldavis_hip.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and header disagree"


def test_struct_layouts_match_header():
    import ctypes as C
    from rtldavis_amd import _lib
    assert C.sizeof(_lib.RdConfig) == 5 * 4 + 64
    assert C.sizeof(_lib.RdPacket) == 4 * 4 + 32 + 2 * 8
    assert _lib.RdPacket.data.offset == 16 and _lib.RdPacket.rssi.offset == 48
    assert C.sizeof(_lib.RdTiming) == 24
    assert C.sizeof(_lib.RdParsed) == 6 * 4 + 32 + 2 * 8
    assert C.sizeof(_lib.RdChanConfig) == 4 * 4 + 8 and _lib.RdChanConfig.gain.offset == 16


def test_packet_config_mirrors_reference():
    from rtldavis_amd import dsp
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    assert (cfg.sample_rate, cfg.block_size2, cfg.preamble_length, cfg.packet_length, cfg.buffer_length) == \
        (268800, 16384, 224, 1120, 16384)
    assert cfg.preamble_str == bytes([1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1])
    assert dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001").buffer_length == 2048  # default block 512


def test_argument_errors_without_gpu():
    """Size checks come before any device work (dsp.py:32-36,145-149)."""
    from rtldavis_amd import dsp
    dem = dsp.Demodulator(dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192))  # no HIP init here
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        dem.demodulate(np.zeros(7, dtype=np.uint8))
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        dem.demodulate(np.zeros(7, dtype=np.complex64))
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        dsp.ByteToCmplxLUT().execute(np.zeros(10, np.uint8), np.zeros(4, np.complex128))
    with pytest.raises(ValueError):
        dsp.Demodulator(dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 30))  # not a multiple of 4


def test_create_argument_checks_without_gpu():
    """Bad shapes/configs are rejected by the host part of the C ABI before any device work."""
    import ctypes as C
    from rtldavis_amd import _lib, batch, dsp
    good = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    for ns, nb in [(0, 1), (1, 0), (-3, 2)]:
        with pytest.raises(ValueError):
            batch.BatchDemodulator(good, ns, nb)
    with pytest.raises(ValueError):  # packet shorter than the preamble
        batch.BatchDemodulator(dsp.PacketConfig(19200, 14, 16, 8, "1100101110001001", 8192), 1, 1)
    with pytest.raises(ValueError):  # preamble symbols must be 0/1
        dsp.Demodulator(dsp.PacketConfig(19200, 14, 4, 80, "1120", 512))
    with pytest.raises(ValueError):
        dsp.MultiDemodulator(good, 0)
    h = C.c_void_p()
    assert _lib.lib().rd_create(None, C.byref(h)) == _lib.RD_ERR_ARG
    assert b"null config" in _lib.lib().rd_last_error()
    # results before run is a state error, not a crash
    b = batch.BatchDemodulator(good, 1, 1)
    n = C.c_int()
    assert _lib.lib().rd_batch_results(b._b, None, 0, C.byref(n)) in (_lib.RD_ERR_STATE, _lib.RD_ERR_DEVICE)


def test_batch_size_limit_at_its_edge():
    """rd_batch_create (host only, allocates nothing): a batch holds at most 0x0FFFFFFF 32-sample runs - a fix-up
    entry's word index has 28 bits.  The limit itself is accepted, one more stream is RD_ERR_ARG; for the production
    block size, where a stream's run count is even and the limit odd, the nearest count below it."""
    import ctypes as C
    from rtldavis_amd import _lib, dsp
    from rtldavis_amd.dsp import _cfg_struct
    L = _lib.lib()
    limit = 0x0FFFFFFF

    def create(cfg, ns, nb):
        h = C.c_void_p()
        rc = L.rd_batch_create(C.byref(_cfg_struct(cfg)), ns, nb, C.byref(h))
        msg = L.rd_last_error() if rc else b""
        if h:
            L.rd_batch_destroy(h)
        return rc, msg

    # block_size 36, 2 blocks: 72 samples = 3 runs per stream, and 3 divides the limit
    small = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 36)
    prod = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    for cfg, nb in ((small, 2), (prod, 33), (prod, 1)):
        runs = (nb * cfg.block_size + 31) // 32
        ns = limit // runs
        assert ns * runs <= limit < (ns + 1) * runs
        assert create(cfg, ns, nb) == (_lib.RD_OK, b""), (cfg.block_size, nb)
        rc, msg = create(cfg, ns + 1, nb)
        assert rc == _lib.RD_ERR_ARG and b"batch too large" in msg, (cfg.block_size, nb, rc, msg)
    assert (limit // 3) * 3 == limit   # the first case sits on the limit exactly


def test_no_silent_cpu_fallback():
    """Without a GPU every compute entry point must raise, never return numbers."""
    from rtldavis_amd import _lib, batch, dsp
    if _lib.lib().rd_device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    with pytest.raises(_lib.HipError):
        dsp.Demodulator(cfg).demodulate(np.zeros(16384, dtype=np.uint8))
    with pytest.raises(_lib.HipError):
        batch.BatchDemodulator(cfg, 2, 2).demodulate(np.zeros((2, 32768), dtype=np.uint8))
    with pytest.raises(_lib.HipError):
        dsp.quantize(np.zeros(4), np.zeros(4, np.uint8))


def test_channelizer_argument_checks_and_no_fallback():
    """rd_chan_create validates without touching the device; without a GPU the compute calls raise."""
    from rtldavis_amd import _lib, channelizer
    with pytest.raises(ValueError):
        channelizer.Channelizer([914963100], centre_hz=914963100, decim=0)          # no decimation factor
    with pytest.raises(ValueError):
        channelizer.Channelizer([902419338], centre_hz=990000000)                   # outside the captured band
    with pytest.raises(ValueError):
        channelizer.Channelizer([914963100], gain=0.0)
    with pytest.raises(ValueError):
        channelizer.Channelizer([914963100], taps=np.ones(9000))                    # more taps than the kernel stages
    with pytest.raises(ValueError):
        channelizer.Channelizer([914963100], decim=98)                              # decimation not a multiple of 4
    cz = channelizer.Channelizer()                                                  # host state only
    assert cz.n_channels == 51 and cz.shift_hz[25] == 67200 and cz.taps.size == 512
    if _lib.lib().rd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.HipError):
        cz.upload(np.zeros(2 * 100 * 64, np.uint8))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "rtldavis_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "dsp_oracle" not in text, f


def test_shard_ranges_cover_and_balance():
    from rtldavis_amd.shard import shard_range
    for n, w in [(32768, 8), (4096, 3), (5, 8), (51, 4), (1, 1)]:
        parts = [shard_range(n, w, r) for r in range(w)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        sizes = [hi - lo for lo, hi in parts]
        assert max(sizes) - min(sizes) <= 1


def test_traffic_stamp_of_the_built_demod_kernel():
    """bench.py accepts a profiles/rNN_traffic.json only when its stamp equals the one the build left next to the
    library: a sha256 over the instructions of k_demod_mfma (tools/profile_collect.py::isa_sha256 - the kernel's body
    in hipcc's device assembly, comments and label numbers dropped)."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("profile_collect", os.path.join(ROOT, "tools", "profile_collect.py"))
    pc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pc)
    stamp = pc.kernel_isa_stamp()
    assert len(stamp) == 64 and int(stamp, 16) >= 0, "make -C rtldavis_amd/csrc all writes librtldavis_hip.stamp"
    asm = "\n".join(["_Z5otherv:", "\ts_endpgm", pc.DEMOD_KERNEL_SYMBOL + "v9rd_layout: ; @k", "; %bb.0:", "\ts_load_dword s0, s[4:5], 0x0 ; c",
                     ".LBB7_2:", "\ts_cbranch_scc1 .LBB7_2", "\ts_endpgm", "\t.section x"])
    again = asm.replace("LBB7_", "LBB3_").replace("; c", "; another comment")
    assert pc.isa_sha256(asm) == pc.isa_sha256(again) != ""
    assert pc.isa_sha256(asm.replace("0x0", "0x4")) != pc.isa_sha256(asm)
    assert pc.isa_sha256("_Z5otherv:\n\ts_endpgm\n") == ""
    with open(os.path.join(ROOT, "profiles", "r03_traffic.json")) as fh:
        tj = json.load(fh)
    assert len(tj["kernel_isa_sha256"]) == 64 and tj["traffic_bytes"] > tj["algorithmic_bytes"]


def test_isa_kernels_lines_follow_the_code_not_its_place():
    """tools/profile_collect.py::isa_kernels, the per-kernel comparison of two builds: a kernel's line (symbol, sha256 of
    its instructions, their count, the figures of its .amdhsa_ block) does not depend on the file's order, its label
    numbers or its comments, and one changed operand changes exactly that kernel's hash."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("profile_collect", os.path.join(ROOT, "tools", "profile_collect.py"))
    pc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pc)

    def kernel(name, n, offset, note, vgpr):
        return ["\t.type\t%s,@function" % name, "%s: ; @%s" % (name, name), "; %bb.0:", "\ts_load_dword s0, s[4:5], %s ; %s" % (offset, note),
                ".LBB%d_2: ; %s" % (n, note), "\tv_add_u32_e32 v0, s0, v0", "\ts_cbranch_scc1 .LBB%d_2" % n, "\ts_endpgm", ".Lfunc_end%d:" % n,
                "\t.section\t.rodata", "\t.amdhsa_kernel %s" % name, "\t\t.amdhsa_group_segment_fixed_size 48",
                "\t\t.amdhsa_private_segment_fixed_size 0", "\t\t.amdhsa_next_free_vgpr %d" % vgpr, "\t\t.amdhsa_next_free_sgpr 20",
                "\t\t.amdhsa_accum_offset 8", "\t.end_amdhsa_kernel", "\t.text"]

    def text(order, offset_a="0x0", note="c"):
        parts = {"a": kernel("_Z3k_av", 3 if order == "ab" else 9, offset_a, note, 6),
                 "b": kernel("_Z3k_bv", 4 if order == "ab" else 1, "0x8", note, 7)}
        return "\n".join(["\t.text"] + parts[order[0]] + parts[order[1]] + ["_Z6helperv:", "\ts_setpc_b64 s[30:31]"])

    one, two = pc.isa_kernels(text("ab")), pc.isa_kernels(text("ba", note="another comment"))
    assert one == two and [ln.split()[0] for ln in one] == ["_Z3k_av", "_Z3k_bv"]
    name, sha, count, *figures = one[0].split()
    assert len(sha) == 64 and count == "4" and figures == ["vgpr=6", "sgpr=20", "private=0", "lds=48", "accum=8"]
    assert one[1].split()[2:] == ["4", "vgpr=7", "sgpr=20", "private=0", "lds=48", "accum=8"] and one[1].split()[1] != sha
    changed = pc.isa_kernels(text("ab", offset_a="0x4"))
    assert changed[0].split()[1] != sha and changed[0].split()[2:] == one[0].split()[2:] and changed[1] == one[1]


def _refusal_env():
    import ctypes as C
    from rtldavis_amd import _lib, dsp
    from rtldavis_amd.dsp import _cfg_struct
    L = _lib.lib()
    cfg = _cfg_struct(dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 512))
    handles = {}
    for name, ns in (("h1", 1), ("h3", 3)):
        h = C.c_void_p()
        assert L.rd_create_multi(C.byref(cfg), ns, C.byref(h)) == _lib.RD_OK
        handles[name] = h
    return C, _lib, L, cfg, handles


def test_streaming_refusals_decided_before_any_device_call():
    """Every argument and state refusal of the streaming entry points that is decided before a device call, on fresh
    handles (rd_create is lazy: no GPU needed) of block_size 512 - B = 512, L = 2048 - with one stream and with three:
    the return code and the whole rd_last_error text, and which refusal wins where two apply."""
    C, _lib, L, _, hs = _refusal_env()
    h1, h3 = hs["h1"], hs["h3"]
    ARG, STATE, OK = _lib.RD_ERR_ARG, _lib.RD_ERR_STATE, _lib.RD_OK
    buf = np.ones(4 * 3072, np.float64)        # never read: every row below is refused first
    p = buf.ctypes.data_as(C.c_void_p)
    n = C.c_int(-7)
    pn = C.byref(n)
    sizes = "Incompatible array sizes: got %d, expected %d"
    rows = [
        # rd_demod_submit(h, samples, count, is_complex)
        (L.rd_demod_submit, (None, p, 1024, 0), ARG, "null argument"),
        (L.rd_demod_submit, (h1, None, 1024, 0), ARG, "null argument"),
        (L.rd_demod_submit, (h1, p, 1023, 0), ARG, sizes % (1023, 1024)),
        (L.rd_demod_submit, (h1, p, 512, 0), ARG, sizes % (512, 1024)),
        (L.rd_demod_submit, (h1, p, 1024, 1), ARG, sizes % (1024, 512)),
        (L.rd_demod_submit, (h1, p, 0, 1), ARG, sizes % (0, 512)),
        (L.rd_demod_submit, (h3, p, 1024, 0), ARG, sizes % (1024, 3072)),
        (L.rd_demod_submit, (h3, p, 512, 1), STATE, "complex input needs a single-stream handle"),
        (L.rd_demod_submit, (h3, p, 7, 1), STATE, "complex input needs a single-stream handle"),   # (before the size)
        (L.rd_demod_submit, (h3, None, 7, 1), ARG, "null argument"),                                 # (before both)
        # rd_demod_submit_from(h, offset, count, is_complex): no buffer registered, whatever else is wrong
        (L.rd_demod_submit_from, (None, 0, 1024, 0), ARG, "null handle"),
        (L.rd_demod_submit_from, (h1, 0, 1024, 0), STATE, "no input buffer registered (rd_demod_register_input)"),
        (L.rd_demod_submit_from, (h1, 8, 1000, 0), STATE, "no input buffer registered (rd_demod_register_input)"),
        (L.rd_demod_submit_from, (h3, 0, 512, 1), STATE, "no input buffer registered (rd_demod_register_input)"),
        # rd_demod_block(h, samples, count, is_complex, out, cap, n)
        (L.rd_demod_block, (None, p, 1024, 0, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_block, (h1, None, 1024, 0, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_block, (h1, p, 1024, 0, None, 0, None), ARG, "null argument"),
        (L.rd_demod_block, (h3, p, 3072, 0, None, 0, pn), STATE, "handle holds 3 streams: use rd_demod_blocks"),
        (L.rd_demod_block, (h3, p, 5, 1, None, 0, pn), STATE, "handle holds 3 streams: use rd_demod_blocks"),   # (before the size)
        (L.rd_demod_block, (h1, p, 1000, 0, None, 0, pn), ARG, sizes % (1000, 1024)),
        (L.rd_demod_block, (h1, p, 1024, 1, None, 0, pn), ARG, sizes % (1024, 512)),
        (L.rd_demod_block, (h1, p, 513, 1, None, 0, pn), ARG, sizes % (513, 512)),
        # rd_demod_blocks(h, iq, nbytes, out, cap, n): the one that says "bytes"
        (L.rd_demod_blocks, (None, p, 1024, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_blocks, (h1, None, 1024, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_blocks, (h1, p, 1024, None, 0, None), ARG, "null argument"),
        (L.rd_demod_blocks, (h1, p, 1000, None, 0, pn), ARG, "Incompatible array sizes: got 1000 bytes, expected 1024"),
        (L.rd_demod_blocks, (h3, p, 1024, None, 0, pn), ARG, "Incompatible array sizes: got 1024 bytes, expected 3072"),
        (L.rd_demod_blocks, (h3, p, 3073, None, 0, pn), ARG, "Incompatible array sizes: got 3073 bytes, expected 3072"),
        # fetch / parsed / set_parse on a handle that has seen no block
        (L.rd_demod_fetch, (None, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_fetch, (h1, None, 0, None), ARG, "null argument"),
        (L.rd_demod_fetch, (h1, None, 0, pn), STATE, "no block in flight"),
        (L.rd_demod_fetch, (h3, None, 0, pn), STATE, "no block in flight"),
        (L.rd_demod_refetch, (None, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_refetch, (h1, None, 0, None), ARG, "null argument"),
        (L.rd_demod_parsed, (None, None, 0, pn), ARG, "null argument"),
        (L.rd_demod_parsed, (h1, None, 0, None), ARG, "null argument"),
        (L.rd_demod_parsed, (h1, None, 0, pn), STATE, "no block fetched since create / reset"),
        (L.rd_demod_set_parse, (None, 1), ARG, "null handle"),
        # state accessors: rd_copy_discriminated_stream(h, stream, out, n), rd_copy_filtered(h, out, n), rd_copy_quantized(h, out, n)
        (L.rd_copy_discriminated_stream, (None, 0, p, 1024), ARG, "null argument"),
        (L.rd_copy_discriminated_stream, (h1, 0, None, 1024), ARG, "null argument"),
        (L.rd_copy_discriminated_stream, (h1, 1, p, 1024), ARG, "stream out of range"),
        (L.rd_copy_discriminated_stream, (h1, -1, p, 1024), ARG, "stream out of range"),
        (L.rd_copy_discriminated_stream, (h3, 3, p, 7), ARG, "stream out of range"),                 # (before the size)
        (L.rd_copy_discriminated_stream, (h3, 2, p, 1023), ARG, "discriminated has 1024 elements"),
        (L.rd_copy_discriminated, (None, p, 1024), ARG, "null argument"),
        (L.rd_copy_discriminated, (h1, p, 512), ARG, "discriminated has 1024 elements"),
        (L.rd_copy_filtered, (None, p, 513), ARG, "null argument"),
        (L.rd_copy_filtered, (h1, None, 513), ARG, "null argument"),
        (L.rd_copy_filtered, (h1, p, 512), ARG, "filtered has 513 elements"),
        (L.rd_copy_filtered, (h3, p, 1026), ARG, "filtered has 513 elements"),
        (L.rd_copy_quantized, (None, p, 2048), ARG, "null argument"),
        (L.rd_copy_quantized, (h1, None, 2048), ARG, "null argument"),
        (L.rd_copy_quantized, (h1, p, 1024), ARG, "quantized has 2048 elements"),
        (L.rd_copy_quantized, (h3, p, 2049), ARG, "quantized has 2048 elements"),
    ]
    for fn, args, code, text in rows:
        rc = fn(*args)
        assert (rc, L.rd_last_error().decode()) == (code, text), (fn.__name__, args[1:])
    assert n.value == -7                                   # no refusal wrote a count
    # what a fresh handle answers without a device: no packets, all-zero state (dsp.py:134-135)
    for h in (h1, h3):
        assert L.rd_demod_inflight(h) == 0
        assert L.rd_demod_refetch(h, None, 0, pn) == OK and n.value == 0
        n.value = -7
        for enabled in (1, 0):                             # parse may be switched on a quiet handle; still nothing fetched
            assert L.rd_demod_set_parse(h, enabled) == OK
            assert (L.rd_demod_parsed(h, None, 0, pn), L.rd_last_error().decode()) == (STATE, "no block fetched since create / reset")
        d = np.ones(1024)
        assert L.rd_copy_discriminated_stream(h, 0, d.ctypes.data_as(C.c_void_p), 1024) == OK and not d.any()
        f = np.ones(2 * 513)
        assert L.rd_copy_filtered(h, f.ctypes.data_as(C.c_void_p), 513) == OK and not f.any()
        q = np.ones(2048, np.uint8)
        assert L.rd_copy_quantized(h, q.ctypes.data_as(C.c_void_p), 2048) == OK and not q.any()
    d = np.ones(1024)
    assert L.rd_copy_discriminated(h1, d.ctypes.data_as(C.c_void_p), 1024) == OK and not d.any()
    d = np.ones(1024)
    assert L.rd_copy_discriminated_stream(h3, 2, d.ctypes.data_as(C.c_void_p), 1024) == OK and not d.any()
    for h in (h1, h3):
        L.rd_destroy(h)


def test_stage_function_refusals_decided_before_any_device_call():
    """The stage functions' argument refusals (and the empty calls that succeed without a device): code and whole text,
    and the size rule before the null check where both apply."""
    C, _lib, L, cfg, hs = _refusal_env()
    for h in hs.values():
        L.rd_destroy(h)
    ARG, OK = _lib.RD_ERR_ARG, _lib.RD_OK
    buf = np.ones(4096)
    p = buf.ctypes.data_as(C.c_void_p)
    cnt = C.c_int(-7)
    pc = C.byref(cnt)
    bad = type(cfg)()
    C.memmove(C.byref(bad), C.byref(cfg), C.sizeof(cfg))
    bad.symbol_length = 0
    rows = [
        (L.rd_lut_execute, (p, 10, p, 4), ARG, "Incompatible array sizes: in_bytes.size=10, out_cplx.size=4"),
        (L.rd_lut_execute, (None, 10, None, 4), ARG, "Incompatible array sizes: in_bytes.size=10, out_cplx.size=4"),
        (L.rd_lut_execute, (p, 0, p, 0), OK, None),
        (L.rd_lut_execute, (None, 8, p, 4), ARG, "null argument"),
        (L.rd_lut_execute, (p, 8, None, 4), ARG, "null argument"),
        (L.rd_rotate_fs4, (None, None, 0), OK, None),
        (L.rd_rotate_fs4, (None, p, 4), ARG, "null argument"),
        (L.rd_rotate_fs4, (p, None, 4), ARG, "null argument"),
        (L.rd_fir9, (p, 8, p, 0), ARG, "fir9: n_out must be <= n_in - 8"),
        (L.rd_fir9, (p, 10, p, 3), ARG, "fir9: n_out must be <= n_in - 8"),
        (L.rd_fir9, (None, 10, None, 3), ARG, "fir9: n_out must be <= n_in - 8"),
        (L.rd_fir9, (None, 9, None, 0), OK, None),
        (L.rd_fir9, (None, 10, p, 2), ARG, "null argument"),
        (L.rd_fir9, (p, 10, None, 2), ARG, "null argument"),
        (L.rd_discriminate, (p, 0, p, 0), ARG, "discriminate: n_out must be n_in - 1"),
        (L.rd_discriminate, (p, 5, p, 3), ARG, "discriminate: n_out must be n_in - 1"),
        (L.rd_discriminate, (None, 5, None, 5), ARG, "discriminate: n_out must be n_in - 1"),
        (L.rd_discriminate, (None, 1, None, 0), OK, None),
        (L.rd_discriminate, (None, 5, p, 4), ARG, "null argument"),
        (L.rd_discriminate, (p, 5, None, 4), ARG, "null argument"),
        (L.rd_quantize, (None, None, 0), OK, None),
        (L.rd_quantize, (None, p, 4), ARG, "null argument"),
        (L.rd_quantize, (p, None, 4), ARG, "null argument"),
        # rd_search(cfg, quantized, n, indices, cap, count); a preamble spans (16 - 1) * 14 = 210 samples
        (L.rd_search, (C.byref(cfg), p, 4096, p, 0, None), ARG, "null count"),
        (L.rd_search, (None, p, 4096, p, 0, pc), ARG, "null config"),
        (L.rd_search, (None, p, 4096, p, 0, None), ARG, "null count"),
        (L.rd_search, (C.byref(bad), p, 4096, p, 0, pc), ARG, "unsupported packet configuration"),
        (L.rd_search, (C.byref(cfg), None, 211, p, 0, pc), ARG, "null argument"),
    ]
    for fn, args, code, text in rows:
        rc = fn(*args)
        assert rc == code, (fn.__name__, args, rc, L.rd_last_error())
        if text is not None:
            assert L.rd_last_error().decode() == text, (fn.__name__, args)
    cnt.value = -7
    assert L.rd_search(C.byref(cfg), None, 210, None, 0, pc) == OK and cnt.value == 0   # too short to hold a preamble
