"""C-ABI surface: librd_hip.so loads without a GPU and exports every symbol include/ribodetector_amd.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _declared():
    src = open(os.path.join(ROOT, "include", "ribodetector_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    from ribodetector_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(N.LIB_PATH)
    declared = _declared()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), "librd_hip.so does not export %s" % name
    assert sorted(N.SYMBOLS) == declared, "ribodetector_amd/_native.py binding list differs from the header"
    assert b"gfx950" in N.lib().rd_version()


def test_host_library_symbols():
    from ribodetector_amd import _native as N
    src = open(os.path.join(ROOT, "include", "ribodetector_amd_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", src)))
    lib = ctypes.CDLL(N.HOST_LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), "librd_host.so does not export %s" % name
    assert sorted(N.HOST_SYMBOLS) == declared


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_libraries_export_the_headers_and_nothing_else():
    """nm -D of both libraries = the headers' declarations, exactly: internal helpers, libstdc++ instantiations and the HIP
    compilation-unit id stay local (-fvisibility=hidden + csrc/rd_exports.map)"""
    import shutil
    if not shutil.which("nm"):
        pytest.skip("binutils nm not installed")
    from ribodetector_amd import _native as N
    assert _exported(N.LIB_PATH) == sorted(N.SYMBOLS)
    assert _exported(N.HOST_LIB_PATH) == sorted(N.HOST_SYMBOLS)


def test_missing_extension_fails_loudly(monkeypatch):
    from ribodetector_amd import _native as N
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(N, "LIB_PATH", "/nonexistent/librd_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.lib()


def test_argument_errors_without_gpu():
    """argument validation paths that return before any HIP call"""
    from ribodetector_amd import _native as N
    L = N.lib()
    assert L.rd_classify_workspace_bytes(1000, 100) > 0
    assert L.rd_classify_workspace_bytes(-1, 100) == 0
    rc = L.rd_model_create(None, 0, None)
    assert rc == -1 and b"null" in L.rd_last_error()
    rc = L.rd_pair_fuse(None, None, 5, 7, None, None, None)
    assert rc == -1
    # sibling entry points share their validation: the same bad arguments give the same code from both, and the message names the
    # entry point that was called. No pointer is dereferenced before the checks: P / Q stand for an aligned / a misaligned one.
    # (Every case below must be refused: a call that passed the checks would launch kernels on these addresses.)
    P, Q, big = 0x10000, 0x10001, 1 << 40

    def refused(name, args, code, word):
        rc = getattr(L, name)(*args)
        msg = L.rd_last_error()
        assert rc == code and msg.startswith(name.encode() + b":") and word in msg, (name, args, rc, msg)

    def gzs(comp=P, comp_bytes=4096, data=2048, valid=2048, section=1024, cap=1024, carry=None, carried=None, out=P, ws=P, ws_bytes=big):
        return (comp, comp_bytes, data, valid, section, cap, 0, carry, 0, 0, carried, P, out, 1 << 16, P, ws, ws_bytes, None)
    for name in ("rd_gz_stream_inflate", "rd_gz_range_decode"):
        refused(name, gzs(comp=None), -1, b"null")
        refused(name, gzs(ws=None), -1, b"null")
        refused(name, gzs(ws=Q), -1, b"aligned")
        refused(name, gzs(out=Q), -1, b"aligned")
        refused(name, gzs(data=0), -1, b"bad sizes")
        refused(name, gzs(valid=1024), -1, b"bad sizes")
        refused(name, gzs(section=1022), -1, b"bad sizes")
        refused(name, gzs(ws_bytes=0), -4, b"workspace too small")
    refused("rd_gz_stream_inflate", gzs(out=P + 8, ws_bytes=0), -4, b"workspace too small")   # (text: 8-byte aligned will do)
    refused("rd_gz_range_decode", gzs(out=P + 8), -1, b"sym_text 16-byte aligned")
    refused("rd_gz_range_decode", gzs(carry=P), -1, b"carry and map_in go together")
    refused("rd_gz_range_decode", gzs(carried=P), -1, b"carry and map_in go together")

    def index(name, text=P, pad=64, end=4096, prev_text=None, prev=None, norm=P, ws=P, ws_bytes=big):
        fa = (norm, 1 << 16, P, P, 64) if name == "rd_fasta_index" else ()
        return (text, pad, end, prev_text, prev, 0, P, 1024) + fa + (P, ws, ws_bytes, None)
    for name in ("rd_fastq_index", "rd_fasta_index"):
        refused(name, index(name, text=None), -1, b"null")
        refused(name, index(name, ws=None), -1, b"null")
        refused(name, index(name, end=63), -1, b"bad pad / end")
        refused(name, index(name, pad=-1), -1, b"bad pad / end")
        refused(name, index(name, prev_text=P), -1, b"prev and prev_text go together")
        refused(name, index(name, prev=P), -1, b"prev and prev_text go together")
        refused(name, index(name, ws=Q), -1, b"aligned")
        refused(name, index(name, text=P + 32), -1, b"aligned")
        refused(name, index(name, ws_bytes=0), -4, b"workspace too small")
    refused("rd_fasta_index", index("rd_fasta_index", norm=None), -1, b"null")
    refused("rd_fasta_index", index("rd_fasta_index", norm=Q), -1, b"norm 16-byte aligned")

    def gather(name, src=P, lo=0, hi=8, out=P, cur_out=P + 8):
        return ((src, P, P) if name == "rd_fasta_gather" else (src, P)) + (P, lo, hi, 4096, out, 4096, P, cur_out, P, P, P, None)
    for name in ("rd_fastq_gather", "rd_fasta_gather"):
        refused(name, gather(name, src=None), -1, b"null")
        refused(name, gather(name, out=None), -1, b"null")
        refused(name, gather(name, lo=9), -1, b"bad range")
        refused(name, gather(name, cur_out=P), -1, b"bad range")
        refused(name, gather(name, out=Q), -1, b"aligned")
    for name in ("rd_fastq_sample", "rd_fasta_sample"):
        refused(name, (None, P, 4096, P, 8, None), -1, b"bad argument")
        refused(name, (P, P, 0, P, 8, None), -1, b"bad argument")
        refused(name, (P, P, 4096, P, -1, None), -1, b"bad argument")

    def select(text=P, tb=1000, n=10, label=0, out=P, info=P, ws=P, ws_bytes=big):
        return (text, tb, P, P, n, label, out, 1 << 20, info, ws, ws_bytes, None)
    for name in ("rd_gz_compress_selected", "rd_select_pack"):
        refused(name, select(n=-1), -1, b"bad n")
        refused(name, select(tb=-1), -1, b"bad n")
        refused(name, select(info=None), -1, b"null")
        refused(name, select(label=128), -1, b"int8")
        refused(name, select(label=-129), -1, b"int8")
        refused(name, select(text=None), -1, b"null")
        refused(name, select(out=None), -1, b"null")
        refused(name, select(ws=None), -1, b"null")
        refused(name, select(ws=Q), -1, b"aligned")
        refused(name, select(out=Q), -1, b"aligned")
        refused(name, select(ws_bytes=0), -4, b"workspace too small")
    refused("rd_gz_compress_selected", select(out=P + 16), -1, b"aligned")                # (the deflate's output: 256-byte aligned)
    refused("rd_select_pack", select(out=P + 16, ws_bytes=0), -4, b"workspace too small")  # (plain text: 16-byte aligned will do)


# What every sizing function of the C ABI returned before the workspaces were carved by one walk each (csrc/rd_common.hpp Carver):
# (arguments, bytes) at 0, 1, one below / at / above the boundaries a layout rounds to (256-byte pieces of 2- / 4- / 8-byte entries;
# 2,048 items per scan, sort or FASTA line block; 65,280 bytes per gzip member and 512 members per deflate grid; 16 KiB per FASTQ
# tile; 8,192 symbols / 65,536 text bytes per inflate tile; 32 sections per group), a typical chunk (10^6 reads of 100 / 300 bp:
# 250 / 650 MB of FASTQ text; a 64 MiB stream batch) and the values that are refused with 0.
SIZES = {
    "rd_classify_workspace_bytes": [
        ((1000000, 100), 12199424), ((0, 100), 3072), ((1, 100), 3072), ((31, 100), 3072), ((32, 100), 3072), ((63, 100), 3072), ((64, 100), 3072),
        ((65, 100), 3840), ((2046, 100), 26880), ((2047, 100), 26880), ((2048, 100), 26880), ((2049, 100), 28160), ((4095, 100), 51968),
        ((4096, 100), 51968), ((4097, 100), 52992), ((-1, 100), 0), ((1000000, 0), 0), ((1000000, -1), 0), ((1000000, 1), 12004352),
        ((1000000, 31), 12063232), ((1000000, 32), 12065536), ((1000000, 63), 12126208), ((1000000, 64), 12128512), ((1000000, 300), 12593664),
        ((1000000, 16000), 43554304), ((2049, 300), 32768), ((0, 300), 6912), ((1, 300), 6912), ((31, 300), 6912), ((32, 300), 6912),
        ((63, 300), 6912), ((64, 300), 6912), ((65, 300), 7680), ((2046, 300), 30720), ((2047, 300), 30720), ((2048, 300), 30720),
        ((4095, 300), 56576), ((4096, 300), 56576), ((4097, 300), 58624), ((1000000, 300), 12593664),
    ],
    "rd_fasta_index_workspace_bytes": [
        ((104857600, 13111296), 104967936), ((0, 13111296), 104942336), ((1, 13111296), 104942336), ((16383, 13111296), 104942336),
        ((16384, 13111296), 104942336), ((1048575, 13111296), 104942336), ((1048576, 13111296), 104942592), ((2147483646, 13111296), 105466368),
        ((2147483647, 13111296), 0), ((-1, 13111296), 0), ((104857600, 0), 26368), ((104857600, 1), 26880), ((104857600, 63), 26880),
        ((104857600, 64), 26880), ((104857600, 65), 27392), ((104857600, 2047), 42752), ((104857600, 2048), 42752), ((104857600, 2049), 43264),
        ((104857600, 65536), 550656), ((104857600, 65537), 551424), ((104857600, 104857602), 839297280), ((104857600, -1), 0), ((0, 0), 768),
        ((1, 1), 1280), ((16384, 2049), 17664),
    ],
    "rd_fastq_index_workspace_bytes": [
        ((0,), 256), ((1,), 256), ((16382,), 256), ((16383,), 256), ((16384,), 256), ((16385,), 256), ((1048574,), 256), ((1048575,), 256),
        ((1048576,), 512), ((104857600,), 25856), ((2147483646,), 524288), ((2147483647,), 0), ((-1,), 0),
    ],
    "rd_gz_out_bound": [
        ((0,), 0), ((1,), 32), ((65279,), 65310), ((65280,), 65311), ((65281,), 65343), ((33423359,), 33439231), ((33423360,), 33439232),
        ((33423361,), 33439264), ((250000000,), 250118730), ((650000000,), 650308698), ((-1,), 0),
    ],
    "rd_gz_range_resolve_workspace_bytes": [
        ((0,), 256), ((1,), 256), ((65535,), 256), ((65536,), 256), ((65537,), 256), ((4063231,), 256), ((4063232,), 256), ((4063233,), 256),
        ((806354944,), 49408), ((-1,), 0),
    ],
    "rd_gz_range_workspace_bytes": [
        ((67108864, 16384, 393216, 806354944), 3506767104), ((0, 16384, 393216, 806354944), 1164800), ((1, 16384, 393216, 806354944), 1164800),
        ((16383, 16384, 393216, 806354944), 1164800), ((16384, 16384, 393216, 806354944), 1164800), ((16385, 16384, 393216, 806354944), 2016768),
        ((524287, 16384, 393216, 806354944), 27576320), ((524288, 16384, 393216, 806354944), 27576320),
        ((524289, 16384, 393216, 806354944), 28559616), ((1032192, 16384, 393216, 806354944), 54118912),
        ((1048576, 16384, 393216, 806354944), 54971904), ((-1, 16384, 393216, 806354944), 0), ((67108864, 1023, 393216, 806354944), 0),
        ((67108864, 1024, 393216, 806354944), 56105551104), ((67108864, 1028, 393216, 806354944), 55887372800),
        ((67108864, 65536, 393216, 806354944), 876827904), ((67108864, 16384, 1023, 806354944), 0), ((67108864, 16384, 1024, 806354944), 293930240),
        ((67108864, 16384, 8191, 806354944), 352642304), ((67108864, 16384, 8192, 806354944), 352650496),
        ((67108864, 16384, 8193, 806354944), 352658688), ((67108864, 16384, 65536, 806354944), 822412544), ((67108864, 16384, 393216, 0), 3506717952),
        ((67108864, 16384, 393216, 1), 3506717952), ((67108864, 16384, 393216, 65535), 3506717952), ((67108864, 16384, 393216, 65536), 3506717952),
        ((67108864, 16384, 393216, 65537), 3506717952), ((67108864, 16384, 393216, 4063232), 3506717952),
        ((67108864, 16384, 393216, 4128768), 3506717952), ((67108864, 16384, 393216, 4128769), 3506718208), ((67108864, 16384, 393216, -1), 0),
        ((1048576, 1024, 1024, 1048576), 73569536), ((0, 1024, 1024, 1048576), 331264), ((1, 1024, 1024, 1048576), 331264),
        ((1023, 1024, 1024, 1048576), 331264), ((1024, 1024, 1024, 1048576), 331264), ((1025, 1024, 1024, 1048576), 398848),
        ((32767, 1024, 1024, 1048576), 2426880), ((32768, 1024, 1024, 1048576), 2426880), ((32769, 1024, 1024, 1048576), 2625792),
        ((1048576, 1024, 1024, 0), 73569536), ((1048576, 1024, 1024, 65536), 73569536),
    ],
    "rd_gz_stream_workspace_bytes": [
        ((67108864, 16384, 393216, 806354944), 3506767104), ((0, 16384, 393216, 806354944), 1164800), ((1, 16384, 393216, 806354944), 1164800),
        ((16383, 16384, 393216, 806354944), 1164800), ((16384, 16384, 393216, 806354944), 1164800), ((16385, 16384, 393216, 806354944), 2016768),
        ((524287, 16384, 393216, 806354944), 27576320), ((524288, 16384, 393216, 806354944), 27576320),
        ((524289, 16384, 393216, 806354944), 28559616), ((1032192, 16384, 393216, 806354944), 54118912),
        ((1048576, 16384, 393216, 806354944), 54971904), ((-1, 16384, 393216, 806354944), 0), ((67108864, 1023, 393216, 806354944), 0),
        ((67108864, 1024, 393216, 806354944), 56105551104), ((67108864, 1028, 393216, 806354944), 55887372800),
        ((67108864, 65536, 393216, 806354944), 876827904), ((67108864, 16384, 1023, 806354944), 0), ((67108864, 16384, 1024, 806354944), 293930240),
        ((67108864, 16384, 8191, 806354944), 352642304), ((67108864, 16384, 8192, 806354944), 352650496),
        ((67108864, 16384, 8193, 806354944), 352658688), ((67108864, 16384, 65536, 806354944), 822412544), ((67108864, 16384, 393216, 0), 3506717952),
        ((67108864, 16384, 393216, 1), 3506717952), ((67108864, 16384, 393216, 65535), 3506717952), ((67108864, 16384, 393216, 65536), 3506717952),
        ((67108864, 16384, 393216, 65537), 3506717952), ((67108864, 16384, 393216, 4063232), 3506717952),
        ((67108864, 16384, 393216, 4128768), 3506717952), ((67108864, 16384, 393216, 4128769), 3506718208), ((67108864, 16384, 393216, -1), 0),
        ((1048576, 1024, 1024, 1048576), 73569536), ((0, 1024, 1024, 1048576), 331264), ((1, 1024, 1024, 1048576), 331264),
        ((1023, 1024, 1024, 1048576), 331264), ((1024, 1024, 1024, 1048576), 331264), ((1025, 1024, 1024, 1048576), 398848),
        ((32767, 1024, 1024, 1048576), 2426880), ((32768, 1024, 1024, 1048576), 2426880), ((32769, 1024, 1024, 1048576), 2625792),
        ((1048576, 1024, 1024, 0), 73569536), ((1048576, 1024, 1024, 65536), 73569536),
    ],
    "rd_gz_workspace_bytes": [
        ((1000000, 250000000), 642769408), ((0, 250000000), 634765568), ((1, 250000000), 634765568), ((31, 250000000), 634765568),
        ((32, 250000000), 634765824), ((63, 250000000), 634765824), ((64, 250000000), 634766080), ((65, 250000000), 634766080),
        ((2046, 250000000), 634781696), ((2047, 250000000), 634781696), ((2048, 250000000), 634781952), ((2049, 250000000), 634781952),
        ((4095, 250000000), 634798080), ((4096, 250000000), 634798336), ((4097, 250000000), 634798336), ((-1, 250000000), 0), ((1000000, 0), 8397056),
        ((1000000, 1), 8397056), ((1000000, 65279), 8397056), ((1000000, 65280), 8397056), ((1000000, 65281), 8788992),
        ((1000000, 33423359), 208681984), ((1000000, 33423360), 208681984), ((1000000, 33423361), 208813312), ((1000000, 650000000), 1444483584),
        ((1000000, -1), 0), ((1, 1), 393216), ((0, 1), 393216), ((31, 1), 393216), ((32, 1), 393472), ((63, 1), 393472), ((64, 1), 393728),
        ((65, 1), 393728), ((2046, 1), 409344), ((2047, 1), 409344), ((2048, 1), 409600), ((2049, 1), 409600), ((4095, 1), 425728),
        ((4096, 1), 425984), ((4097, 1), 425984), ((1000000, 1), 8397056), ((1, 0), 393216), ((1, 65279), 393216), ((1, 65280), 393216),
        ((1, 65281), 785152), ((1, 33423359), 200678144), ((1, 33423360), 200678144), ((1, 33423361), 200809472), ((1, 250000000), 634765568),
        ((1, 650000000), 1436479744),
    ],
    "rd_report_out_bound": [
        ((1000000, 250000000), 285000000), ((0, 250000000), 250000000), ((1, 250000000), 250000035), ((31, 250000000), 250001085),
        ((32, 250000000), 250001120), ((63, 250000000), 250002205), ((64, 250000000), 250002240), ((65, 250000000), 250002275),
        ((2046, 250000000), 250071610), ((2047, 250000000), 250071645), ((2048, 250000000), 250071680), ((2049, 250000000), 250071715),
        ((4095, 250000000), 250143325), ((4096, 250000000), 250143360), ((4097, 250000000), 250143395), ((-1, 250000000), 0),
        ((1000000, 0), 35000000), ((1000000, 1), 35000001), ((1000000, 650000000), 685000000), ((1000000, -1), 0),
    ],
    "rd_report_workspace_bytes": [
        ((0,), 512), ((1,), 1024), ((31,), 1024), ((32,), 1024), ((63,), 1280), ((64,), 1280), ((65,), 1792), ((2046,), 25088), ((2047,), 25088),
        ((2048,), 25088), ((2049,), 25600), ((4095,), 49664), ((4096,), 49664), ((4097,), 50176), ((1000000,), 12004352), ((-1,), 0),
    ],
    "rd_select_workspace_bytes": [
        ((0,), 512), ((1,), 512), ((31,), 512), ((32,), 768), ((63,), 768), ((64,), 1024), ((65,), 1024), ((2046,), 16640), ((2047,), 16640),
        ((2048,), 16896), ((2049,), 16896), ((4095,), 33024), ((4096,), 33280), ((4097,), 33280), ((1000000,), 8004352), ((-1,), 0),
    ],
}


def test_sizing_functions_return_the_recorded_bytes():
    """a layout change shows here before it corrupts memory: callers size their workspaces with these functions"""
    from ribodetector_amd import _native as N
    L = N.lib()
    for name, cases in SIZES.items():
        for args, want in cases:
            assert getattr(L, name)(*args) == want, (name, args)
    assert SIZES["rd_gz_range_workspace_bytes"] == SIZES["rd_gz_stream_workspace_bytes"]


def _weights(N, sd):
    import ctypes as C
    from ribodetector_amd.model.model import STATE_KEYS
    return N.RdWeights(*[sd[k].ctypes.data_as(C.POINTER(C.c_float)) for k in STATE_KEYS], 4, 128, 2)


def test_weights_outside_the_accepted_range_are_refused_without_gpu():
    """rd_model_create checks the weights on the host before its first device call (include/ribodetector_amd.h): a non-finite value
    is RD_E_INVALID and the message names the tensor; max |weight_hh_l0| >= 65504/16 is RD_E_UNSUPPORTED (16 w is stored in fp16:
    such weights used to give inf there and silent NaN logits). SeqModel.load_state_dict raises RuntimeError and keeps its state."""
    import ctypes as C
    import sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import weight_families as WF
    from ribodetector_amd import _native as N
    from ribodetector_amd.model import model as M
    L = N.lib()
    good = WF.family("random_wide")
    assert L.rd_weights_check(C.byref(_weights(N, good))) == 0
    assert L.rd_weights_check(None) == -1
    m = M.SeqModel(4, 128, 1, 2)
    m.load_state_dict(good)

    def refused(sd, rc, *words):
        h = C.c_void_p()
        assert L.rd_model_create(C.byref(_weights(N, sd)), 0, C.byref(h)) == rc and not h.value
        msg = L.rd_last_error().decode()
        assert all(w in msg for w in words), msg
        assert L.rd_weights_check(C.byref(_weights(N, sd))) == rc
        with pytest.raises(RuntimeError, match=words[0]):
            m.load_state_dict(sd)
        assert all(np.array_equal(m._state[k], good[k]) for k in good)

    for key, at in (("rnn.weight_ih_l0", (511, 3)), ("rnn.weight_hh_l0", (0, 0)), ("rnn.bias_hh_l0", (17,)), ("rnn.weight_hh_l0_reverse", (300, 127)),
                    ("rnn.bias_ih_l0_reverse", (511,)), ("out.weight", (1, 255)), ("out.bias", (1,))):
        for bad in (np.nan, np.inf, -np.inf):
            sd = {k: v.copy() for k, v in good.items()}
            sd[key][at] = bad
            refused(sd, -1, key + " holds a non-finite value")
    limit = np.float32(65504.0 / 16.0)
    for w, ok in ((limit, False), (-limit, False), (np.float32(1e6), False), (np.nextafter(limit, np.float32(0)), True)):
        sd = {k: v.copy() for k, v in good.items()}
        sd["rnn.weight_hh_l0"][511, 127] = w
        if ok:
            assert L.rd_weights_check(C.byref(_weights(N, sd))) == 0
        else:
            refused(sd, -3, "weight_hh_l0", "16 w in fp16")
    # large values elsewhere are inside the range: only W_hh goes through fp16
    sd = {k: v.copy() for k, v in good.items()}
    sd["rnn.weight_hh_l0_reverse"][0, 0] = 1e6
    sd["rnn.bias_ih_l0"][5] = -1e6
    assert L.rd_weights_check(C.byref(_weights(N, sd))) == 0


def test_product_build_has_no_diagnostic_variants():
    """librd_hip.so contains the three kernels that compute the function and nothing else: the A/B and diagnostic
    instantiations (ids >= 10, several wrong by design) and the removed id 3 / 5 must be refused."""
    from ribodetector_amd import _native as N
    L = N.lib()
    assert [v for v in range(-2, 64) if L.rd_variant_available(v)] == [0, 1, 2, 4]
    assert sorted(N.VARIANTS.values()) == [0, 1, 2, 4]
    from ribodetector_amd.model import model as M
    m = M.SeqModel(4, 128, 1, 2)
    for name in ("mfma_f16x3_t32_diag_mfmaonly", "mfma_f16x3", "typo"):
        with pytest.raises(RuntimeError, match="unknown kernel variant"):
            m.set_variant(name)


def test_config_rejects_bad_kernel_block(tmp_path):
    """Predictor.load_model refuses a config.json `kernel` block outside the product set - run, not read: the check comes before
    anything touches a device, so it raises the same way on a box without a GPU"""
    import argparse
    import json
    from ribodetector_amd import detect
    from ribodetector_amd.parse_config import ConfigParser
    base = json.load(open(os.path.join(ROOT, "ribodetector_amd", "config.json")))
    base["state_file"] = {k: os.path.join(ROOT, "ribodetector_amd", v) for k, v in base["state_file"].items()}
    args = argparse.Namespace(log=None, chunk_size=None, len=100, ensure="none", deviceid=None, semantics=None)
    for block, msg in (({"variant": "mfma_f16x3_t32_diag_mfmaonly"}, "kernel.variant must be one of"),
                       ({"variant": "typo"}, "kernel.variant must be one of"),
                       ({"semantics": "tpu"}, "kernel.semantics"),
                       ({"refine": 7}, "kernel.refine"),
                       ({"prefix_k": 3}, "kernel.prefix_k"),
                       ({"prefix_k": "big"}, "kernel.prefix_k"),
                       ({"gzip": "fpga"}, "kernel.gzip")):
        cfg = dict(base, kernel=dict(base["kernel"], **block))
        path = tmp_path / "config.json"
        path.write_text(json.dumps(cfg))
        p = detect.Predictor(ConfigParser.from_json(str(path)), args)
        with pytest.raises(RuntimeError, match=msg):
            p.load_model()
    # the shipped block passes the check (and then fails later only for want of a GPU)
    p = detect.Predictor(ConfigParser.from_json(os.path.join(ROOT, "ribodetector_amd", "config.json")), args)
    assert p.kernel_config() == {"variant": "auto", "semantics": "gpu", "refine": 2.5e-4, "prefix_k": None, "gzip": "device"}
    # kernel.prefix_k is the explicit request for a prefix-state table (a bare SeqModel builds none): the key travels to the model
    cfg = dict(base, kernel=dict(base["kernel"], prefix_k=9))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    assert detect.Predictor(ConfigParser.from_json(str(tmp_path / "config.json")), args).kernel_config()["prefix_k"] == 9
