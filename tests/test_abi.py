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
