"""rtldavis_amd - MI355X (gfx950) implementation of rtldavis's IQ -> bits -> packets path.

``rtldavis_amd.dsp`` mirrors ``rtldavis.dsp`` (drop-in for protocol.Parser / worker);
``rtldavis_amd.batch.BatchDemodulator`` demodulates many independent streams per launch;
``rtldavis_amd.WidebandReceiver`` (``rtldavis_amd.wideband``) channelizes and demodulates a live wideband
capture chunk by chunk.  The streaming forms can run ``protocol.Parser.parse``'s front half in their kernels
(``set_parse`` / ``parsed``); ``rtldavis_amd.parse_packet`` is the same CRC gate for one packet on the host.
``rtldavis_amd.track.Tracker`` predicts where a station heard once transmits next (``WidebandReceiver.set_burst_expect``).
``WidebandReceiver.set_burst_search`` finds a station never yet heard, with no energy gate, at every output position.
``WidebandReceiver.set_burst_quality`` measures every burst message's power and noise on the device, and
``rtldavis_amd.burst_packets`` turns the rows into ``dsp.Packet``s with ``rssi`` and ``snr`` for ``protocol.Parser.parse``.
``WidebandReceiver.set_burst_clips`` records the channelized IQ of every burst on the device; ``rtldavis_amd.clips``
(``ClipStitcher``, ``write_sigmf``, ``read_sigmf``) turns the clips into SigMF ``cu8`` recordings, and
``rtldavis_amd.ClipDecoder`` (``rtldavis_amd.replay``) decodes such recordings again on the device, thousands per launch,
under any of the decoder's forms.
"""
__all__ = ["dsp", "batch", "synth", "wideband", "track", "clips", "WidebandReceiver", "parse_packet", "burst_packets",
           "ClipStitcher", "Recording", "write_sigmf", "read_sigmf", "replay", "ClipDecoder"]

import os as _os

# Device->host copies of a few MB (the packet records of a batch) go through the SDMA engines instead
# of a blit kernel: ROCclr's default threshold sends copies below 16 MiB to a compute kernel, which
# has to share the CUs with the persistent demod kernel of the next batch (measured on MI355X: the
# 4 MB readback took 420 us instead of 97 and slowed that kernel by 7 %; whole-step throughput +10 %
# with the SDMA path, profiles/r02_readback_sdma.txt).  Read by the HIP runtime when it initialises,
# so it has to be in the environment before the first HIP call of the process; an explicit setting wins.
if "GPU_FORCE_BLIT_COPY_SIZE" not in _os.environ:
    _os.environ["GPU_FORCE_BLIT_COPY_SIZE"] = "0"
    # Too late when something in this process has initialised HIP already (torch.cuda does on first use): the
    # runtime has read its flags by then and the setting silently does nothing.  Say so once.
    import sys as _sys
    _torch = _sys.modules.get("torch")
    try:
        _late = bool(_torch is not None and _torch.cuda.is_initialized())
    except Exception:  # noqa: BLE001
        _late = False
    if _late:
        import warnings as _warnings
        _warnings.warn("rtldavis_amd: HIP was initialised before this import, so GPU_FORCE_BLIT_COPY_SIZE=0 cannot take "
                       "effect: device-to-host copies of the packet records will run as blit kernels beside the demod "
                       "kernel (about 10 % less batch throughput).  Import rtldavis_amd first, or export "
                       "GPU_FORCE_BLIT_COPY_SIZE=0 in the environment.", RuntimeWarning, stacklevel=2)


def __getattr__(name):
    # (lazy: importing the package loads no submodule, so the environment above is set before anything else runs)
    if name == "WidebandReceiver":
        from .wideband import WidebandReceiver
        return WidebandReceiver
    if name == "burst_packets":
        from .wideband import burst_packets
        return burst_packets
    if name in ("ClipStitcher", "Recording", "write_sigmf", "read_sigmf"):
        from . import clips
        return getattr(clips, name)
    if name == "ClipDecoder":
        from .replay import ClipDecoder
        return ClipDecoder
    if name == "parse_packet":
        from .dsp import parse_packet
        return parse_packet
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
