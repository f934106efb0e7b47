"""SeqModel - drop-in for the reference's `ribodetector.model.model.SeqModel` (model/model.py:10-37) on MI355X.

Same constructor arguments (`config.json: arch.args`), same `load_state_dict` tensor names/shapes, same call:
`model.to('cuda'); model.eval(); logits = model(packed_sequence)` -> fp32 Tensor[B,2] in input order.
The arithmetic runs in hand-written HIP kernels behind the C ABI (include/ribodetector_amd.h); there is no
torch.nn.LSTM inside and no CPU fallback.

Entries:
  * `forward(x: PackedSequence)`  - API parity with the reference (the one-hot tensor is turned back into bases);
  * `forward(x: Tensor[B,L,4])` when built with pack_seq=false - the reference's forward2 (padded input);
  * `classify_bytes(arena, offsets, lens, max_len)` - the native fast entry: raw ASCII reads resident in HBM,
    encoder + recurrence + FC + argmax fused on the device;
  * `classify_windows(arena, offsets, lens, max_len, ...)` - the same for reads of any length: a read longer than max_len is
    classified over several windows of max_len bases and the windows' logits are fused.
"""
import contextlib
import ctypes as C
import logging
import os

import numpy as np
import torch
from torch.nn.utils.rnn import PackedSequence

from .. import _native as N
from .. import windows as W

log = logging.getLogger("ribodetector_amd")


@contextlib.contextmanager
def _device_lock(device):
    """One process at a time sizes and allocates a prefix-state table on a device: ranks that share a GPU would otherwise all read
    the same "free" figure and allocate against it together. An flock on a file named after the device's UUID (advisory, released
    with the process)."""
    import fcntl
    import tempfile
    try:
        uid = str(torch.cuda.get_device_properties(device).uuid)
    except Exception:
        uid = "dev%d" % (device.index if device.index is not None else torch.cuda.current_device())
    path = os.path.join(tempfile.gettempdir(), "rd_prefix_%s.lock" % "".join(ch for ch in uid if ch.isalnum() or ch in "-_"))
    fd = os.open(path, os.O_CREAT | os.O_RDWR, 0o666)
    try:
        fcntl.flock(fd, fcntl.LOCK_EX)
        yield
    finally:
        try:
            fcntl.flock(fd, fcntl.LOCK_UN)
        finally:
            os.close(fd)


STATE_KEYS = ["rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0",
              "rnn.weight_ih_l0_reverse", "rnn.weight_hh_l0_reverse", "rnn.bias_ih_l0_reverse",
              "rnn.bias_hh_l0_reverse", "out.weight", "out.bias"]


class SeqModel:
    def __init__(self, input_size, hidden_size, num_layers, num_classes, batch_first=True, bidirectional=True,
                 pack_seq=True):
        # the kernels cover exactly the shipped architecture (reference config.json:4-15); anything else is an error,
        # never a silent fallback.
        if num_layers != 1:
            raise NotImplementedError("SeqModel: num_layers=%r is not covered by the HIP kernels (only 1)" % (num_layers,))
        if not bidirectional:
            raise NotImplementedError("SeqModel: bidirectional=False is not covered by the HIP kernels")
        if not pack_seq and not batch_first:
            raise NotImplementedError("SeqModel: pack_seq=False needs batch_first=True (the reference's forward2 indexes the "
                                      "batch on dim 0, model/model.py:67-72)")
        if input_size != 4 or hidden_size != 128 or num_classes != 2:
            raise NotImplementedError("SeqModel: kernels are built for input_size=4, hidden_size=128, num_classes=2")
        self.input_size, self.hidden_size, self.num_layers, self.num_classes = input_size, hidden_size, num_layers, num_classes
        self.batch_first, self.bidirectional, self.pack_seq = batch_first, bidirectional, pack_seq
        H4, H = 4 * hidden_size, hidden_size
        self._shapes = dict(zip(STATE_KEYS, [(H4, input_size), (H4, H), (H4,), (H4,), (H4, input_size), (H4, H), (H4,), (H4,),
                                             (num_classes, 2 * H), (num_classes,)]))
        self._state = None
        self._handle = None
        self.device = None
        self._variant = "auto"
        self._semantics = "packed"
        self._refine = None
        self._refine_async = 0
        # prefix-state table (set_prefix_table): none unless asked for - RD_PREFIX_K, config.json kernel.prefix_k (the CLI) or an
        # explicit call; the reference's .to(device) has no side allocations (reference detect.py:93,115-119) and neither has this one
        self._prefix = os.environ.get("RD_PREFIX_K", 0)
        self._prefix_cap = None
        self._ptab = None
        self._ptab_variant = None
        self._ws = None
        self.training = True

    # ---- weights ---------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        sd = {}
        missing = [k for k in STATE_KEYS if k not in state_dict]
        unexpected = [k for k in state_dict if k not in STATE_KEYS]
        if missing or (strict and unexpected):
            raise RuntimeError("Error(s) in loading state_dict for SeqModel: Missing key(s): %s. Unexpected key(s): %s."
                               % (missing, unexpected))
        for k in STATE_KEYS:
            v = state_dict[k]
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != self._shapes[k]:
                raise RuntimeError("size mismatch for %s: got %s, expected %s" % (k, a.shape, self._shapes[k]))
            sd[k] = a
        # the range of weights the kernels can represent (include/ribodetector_amd.h rd_weights_check: host code, no device needed);
        # a refused state dict leaves the model as it was
        N.check(N.lib().rd_weights_check(C.byref(self._weights(sd))), "load_state_dict")
        self._state = sd
        if self._handle is not None:
            self._create()
        return self

    def state_dict(self):
        if self._state is None:
            raise RuntimeError("SeqModel: no weights loaded")
        return {k: torch.from_numpy(v.copy()) for k, v in self._state.items()}

    def _destroy(self):
        if self._handle is not None:
            N.lib().rd_model_destroy(self._handle)
            self._handle = None
        self._ptab = None
        self._ptab_variant = None

    def _weights(self, sd):
        return N.RdWeights(*[sd[k].ctypes.data_as(C.POINTER(C.c_float)) for k in STATE_KEYS],
                           self.input_size, self.hidden_size, self.num_classes)

    def _create(self):
        self._destroy()
        if self._state is None:
            raise RuntimeError("SeqModel.to(): call load_state_dict() first")
        w = self._weights(self._state)
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        N.check(N.lib().rd_model_create(C.byref(w), idx, C.byref(h)), "rd_model_create")
        self._handle = h
        self.set_variant(self._variant)
        self.set_semantics(self._semantics)
        if self._refine is not None:
            self.set_refine(self._refine)
        self.set_prefix_table(self._prefix)
        if self._refine_async:
            self.set_refine_async(self._refine_async)

    def to(self, device, non_blocking=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("SeqModel runs on the GPU only (HIP kernels); got device %r. "
                               "The reference's CPU product is `ribodetector_cpu`." % (device,))
        if not torch.cuda.is_available():
            raise RuntimeError("No visible ROCm/HIP device")
        self.device = device
        self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else "cuda:%d" % device)

    def eval(self):
        self.training = False
        return self

    def set_variant(self, name):
        if name not in N.VARIANTS:
            raise RuntimeError("SeqModel.set_variant: unknown kernel variant %r (this build has: %s)" % (name, ", ".join(sorted(N.VARIANTS))))
        self._variant = name
        if self._handle is not None:
            N.check(N.lib().rd_set_variant(self._handle, N.VARIANTS[name]), "rd_set_variant")
            if self._ptab is not None and self._ptab_variant != self._kernel():
                self.set_prefix_table(self._prefix, self._prefix_cap)   # the rows are the state of the kernel that built them
        return self

    def _kernel(self):
        return "mfma_f16x3_t32" if self._variant == "auto" else self._variant

    def _built_k(self):
        """k of the table in self._ptab ((4^k + 1) KiB), whichever kernel's rows it holds"""
        return 0 if self._ptab is None else (int(self._ptab.numel()) // 1024 - 1).bit_length() // 2

    def set_semantics(self, name):
        """'packed' (default): the reference GPU product, forward1 over min(len, max_len) real timesteps.
        'padded': the reference CPU product `ribodetector_cpu` (model_cpu.forward_last): zero-padded input, gather at the
        last non-zero row. The two differ only for reads shorter than max_len or ending in non-ACGT bases."""
        self._semantics = name
        if self._handle is not None:
            N.check(N.lib().rd_set_semantics(self._handle, N.SEMANTICS[name]), "rd_set_semantics")
        return self

    def set_refine(self, thresh):
        """margin below which a read is re-evaluated in float64 (C ABI rd_set_refine; default 2.5e-4, 0 = off)"""
        self._refine = float(thresh)
        if self._handle is not None:
            N.check(N.lib().rd_set_refine(self._handle, C.c_float(self._refine)), "rd_set_refine")
        return self

    REFINE_DEFAULT = 2.5e-4

    def set_refine_async(self, calls=1):
        """C ABI rd_set_refine_async: classify_bytes only records the reads inside the noise band; the candidates of `calls`
        consecutive calls (1..16; True = 1; 0 / False = the inline pass) are re-evaluated in float64 together on a stream the model
        owns, beside the recurrence of the next call. A call's results are final once `calls` further calls have been issued or
        after sync_results() - see include/ribodetector_amd.h for the buffer contract. forward() (the reference-compatible call)
        always returns final logits."""
        k = 1 if calls is True else 0 if calls is False else int(calls)
        if self._handle is not None:
            self.sync_results()
            N.check(N.lib().rd_set_refine_async(self._handle, k), "rd_set_refine_async")
        self._refine_async = k
        return self

    def sync_results(self):
        """everything issued later on the current stream sees the final results of all earlier classify_bytes calls"""
        if self._handle is not None:
            with torch.cuda.device(self.device):
                N.check(N.lib().rd_sync_results(self._handle, N.stream_ptr(self.device)), "rd_sync_results")
        return self

    def set_prefix_table(self, k="auto", cap=None):
        """Prefix-state table (C ABI rd_set_prefix_table): the recurrence state after every possible sequence of k
        bases, (4^k + 1) KiB of HBM, built in milliseconds by the kernel that will use it (mfma_f16x3_t32 and mfma_f32 each have
        their own rows; `simple` has none); a read then starts k steps in, with bit-identical logits. Opt-in: a model builds no
        table unless this is called (or RD_PREFIX_K / config.json kernel.prefix_k is set; the CLI and bench.py do ask).
        k = 0: none; 4..13: that; "auto": 12 (16 GiB) when table + build scratch (a quarter more) fit a quarter of the free device
        memory, else the largest k that does, else none. `cap` bounds what "auto" picks (the CLI passes the k that pays off for the
        size of its input: building level k costs 4^k steps). If the allocation fails anyway (another process took the memory),
        the next smaller k is tried, down to none - never an exception for want of memory. Sizing and allocation run under a
        per-device lock, so that ranks sharing a GPU do not size against the same free bytes at once."""
        if isinstance(k, str) and k != "auto":
            k = int(k)
        self._prefix = k
        if cap is not None or k != "auto":
            self._prefix_cap = cap
        if self._handle is None:
            return self
        lib = N.lib()
        if self._kernel() not in ("mfma_f16x3_t32", "mfma_f32") and k != 0:
            log.info("prefix-state table: kernel %s has none (k = 0)", self._kernel())
            k = 0
        with torch.cuda.device(self.device), _device_lock(self.device):
            if k == "auto":
                free, _ = torch.cuda.mem_get_info(self.device)
                free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)   # cached blocks are reusable
                k = N.PREFIX_K_AUTO if self._prefix_cap is None else max(0, min(N.PREFIX_K_AUTO, int(self._prefix_cap)))
                while k >= N.PREFIX_K_MIN and int(lib.rd_prefix_table_bytes(k)) + int(lib.rd_prefix_scratch_bytes(k)) > free // 4:
                    k -= 1
                if k < N.PREFIX_K_MIN:
                    k = 0
            k = int(k)
            if k != 0 and not (N.PREFIX_K_MIN <= k <= N.PREFIX_K_MAX):
                raise RuntimeError("SeqModel.set_prefix_table: k must be 0, 'auto' or in [%d, %d]; got %r" % (N.PREFIX_K_MIN, N.PREFIX_K_MAX, k))
            if k == int(lib.rd_prefix_k(self._handle)) and (k == 0 or (self._ptab is not None and self._ptab_variant == self._kernel())):
                return self
            self.sync_results()
            asked = k
            while True:
                tab = scr = None
                if k:
                    try:
                        if self._ptab is not None and self._built_k() == k:
                            tab = self._ptab                        # same size, another kernel's rows: rebuilt in place
                        else:
                            self._ptab = None
                            N.check(lib.rd_set_prefix_table(self._handle, 0, None, 0, None, 0, N.stream_ptr(self.device)), "rd_set_prefix_table")
                            tab = torch.empty(int(lib.rd_prefix_table_bytes(k)), dtype=torch.uint8, device=self.device)
                        scr = torch.empty(int(lib.rd_prefix_scratch_bytes(k)), dtype=torch.uint8, device=self.device)
                    except torch.OutOfMemoryError:
                        tab = scr = None
                        torch.cuda.empty_cache()
                        k = k - 1 if k > N.PREFIX_K_MIN else 0
                        continue
                N.check(lib.rd_set_prefix_table(self._handle, k, N.ptr(tab), 0 if tab is None else tab.numel(), N.ptr(scr),
                                                0 if scr is None else scr.numel(), N.stream_ptr(self.device)), "rd_set_prefix_table")
                self._ptab = tab                         # (the scratch - the level below, a quarter of the table - is released here)
                self._ptab_variant = self._kernel() if k else None
                break
            if k:
                log.info("prefix-state table: k = %d, %d bytes of HBM (+ %d scratch during the build), kernel %s%s", k, tab.numel(),
                         scr.numel(), self._variant, "" if k == asked else " - k = %d did not fit" % asked)
            elif asked:
                log.warning("prefix-state table: not enough device memory for k = %d or any smaller table - none attached", asked)
        return self

    @property
    def prefix_k(self):
        return 0 if self._handle is None else int(N.lib().rd_prefix_k(self._handle))

    def refine(self, arena, offsets, lens, max_len, logits, labels=None, mate_logits=None, thresh=None):
        """float64 re-evaluation (C ABI rd_refine) of the reads whose own margin - or, with `mate_logits`, whose PAIR margin
        (logits + mate_logits, what decides the pair label under --ensure none, reference detect.py:657) - is inside the noise
        band; `logits` (and `labels`) are updated in place on the current stream. thresh None = the model's band (if that is
        0 because the inline pass is switched off: the library default)."""
        n = int(lens.numel())
        if thresh is None:
            thresh = self._refine if self._refine else (0.0 if self._refine is None else self.REFINE_DEFAULT)
        with torch.cuda.device(self.device):
            N.check(N.lib().rd_refine(self._handle, N.ptr(arena), N.ptr(offsets), N.ptr(lens), n, int(max_len), N.ptr(logits),
                                      N.ptr(labels), N.ptr(mate_logits), C.c_float(float(thresh)), N.stream_ptr(self.device)), "rd_refine")
        return logits

    def refine_pairs(self, arena, offsets, lens, max_len, logits, mate_logits, labels=None, thresh=None):
        """one mate of a pair batch: call once per mate, then pair_fuse()"""
        return self.refine(arena, offsets, lens, max_len, logits, labels, mate_logits, thresh)

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # ---- native fast entry --------------------------------------------------------------------------
    def _workspace(self, n, max_len):
        need = int(N.lib().rd_classify_workspace_bytes(n, max_len))
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.device:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.device)
        return self._ws

    def classify_bytes(self, arena, offsets, lens, max_len, want_labels=True, logits=None, labels=None):
        """arena uint8[*] (ASCII), offsets int64[n] (start of read i), lens int32[n]; all on self.device.
        Returns (logits fp32[n,2], labels uint8[n] | None), row i <-> read i. Asynchronous on the current stream."""
        if self._handle is None:
            raise RuntimeError("SeqModel: call .to('cuda') before inference")
        n = int(lens.numel())
        for t, dt, nm in ((arena, torch.uint8, "arena"), (offsets, torch.int64, "offsets"), (lens, torch.int32, "lens")):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise TypeError("classify_bytes: %s must be a contiguous %s CUDA tensor" % (nm, dt))
        if offsets.numel() < n:
            raise ValueError("classify_bytes: offsets shorter than lens")
        if logits is None:
            logits = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        if want_labels and labels is None:
            labels = torch.empty((n,), dtype=torch.uint8, device=self.device)
        ws = self._workspace(n, max_len)
        with torch.cuda.device(self.device):        # the kernels launch on the calling thread's current HIP device
            return self._classify_launch(arena, offsets, lens, n, max_len, logits, labels, want_labels, ws)

    def _classify_launch(self, arena, offsets, lens, n, max_len, logits, labels, want_labels, ws):
        N.check(N.lib().rd_classify(self._handle, N.ptr(arena), N.ptr(offsets), N.ptr(lens), n, int(max_len), N.ptr(logits),
                                    N.ptr(labels if want_labels else None), N.ptr(ws), ws.numel(), N.stream_ptr(self.device)),
                "rd_classify")
        return logits, (labels if want_labels else None)

    # ---- reads longer than max_len over windows (C ABI rd_window_*, csrc/rd_windows.hpp) ------------------------------
    WINDOW_SLICE = 1 << 23          # windows per rd_classify call of classify_window_table: bounds the classify workspace (100 MB at 100 bp)

    def window_plan(self, lens, max_len, stride=None, max_windows=32):
        """First half of classify_windows, on the current stream: the windows of every read counted and scanned (rd_window_plan). Returns
        the plan: a dict with win_first int64[n + 1] on the device and the pinned verdict `info` ({n, windows, 0, fault}), which
        window_table reads once `ready` has passed."""
        if self._handle is None:
            raise RuntimeError("SeqModel: call .to('cuda') before inference")
        if lens.dtype != torch.int32 or not lens.is_cuda or not lens.is_contiguous():
            raise TypeError("classify_windows: lens must be a contiguous torch.int32 CUDA tensor")
        n = int(lens.numel())
        stride, max_windows = W.check_params(max_len, stride, max_windows)
        lib = N.lib()
        win_first = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        info = torch.empty(4, dtype=torch.int64, device=self.device)
        ws = torch.empty(max(int(lib.rd_window_workspace_bytes(n)), 256), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            N.check(lib.rd_window_plan(N.ptr(lens), n, int(max_len), stride, max_windows, N.ptr(win_first), N.ptr(info), N.ptr(ws), ws.numel(),
                                       N.stream_ptr(self.device)), "rd_window_plan")
            host = torch.empty(4, dtype=torch.int64, pin_memory=True).copy_(info, non_blocking=True)
            ready = N.new_event()
            ready.record(torch.cuda.current_stream(self.device))
        return {"n": n, "max_len": int(max_len), "stride": stride, "max_windows": max_windows, "win_first": win_first, "info": host,
                "ready": ready, "keep": (info, ws)}

    def window_table(self, plan, offsets, lens):
        """Second half of the plan: waits (the host, sleeping) for the number of windows - the one host wait of the feature - and
        writes the window table on the current stream (rd_window_fill): plan["win_off"] int64[total], plan["win_len"] int32[total].
        Returns the number of windows."""
        N.wait_event(plan["ready"])
        info = plan["info"]
        if int(info[3]) or int(info[0]) != plan["n"]:
            raise RuntimeError("device window plan: a sequence table entry has a negative length")
        total = int(info[1])
        if offsets.dtype != torch.int64 or not offsets.is_cuda or not offsets.is_contiguous() or offsets.numel() < plan["n"]:
            raise TypeError("classify_windows: offsets must be a contiguous torch.int64 CUDA tensor, one entry per read")
        plan["win_off"] = torch.empty(total, dtype=torch.int64, device=self.device)
        plan["win_len"] = torch.empty(total, dtype=torch.int32, device=self.device)
        plan["total"] = total
        with torch.cuda.device(self.device):
            N.check(N.lib().rd_window_fill(N.ptr(offsets), N.ptr(lens), N.ptr(plan["win_first"]), plan["n"], plan["max_len"], plan["stride"],
                                           plan["max_windows"], total, N.ptr(plan["win_off"]), N.ptr(plan["win_len"]), N.stream_ptr(self.device)),
                    "rd_window_fill")
        return total

    def classify_window_table(self, arena, plan):
        """rd_classify over the window table of a plan, WINDOW_SLICE windows per call, on the current stream: plan["win_logits"]
        fp32[total, 2] (final after sync_results(), like every classify_bytes result)."""
        total = plan["total"]
        out = plan["win_logits"] = torch.empty((total, 2), dtype=torch.float32, device=self.device)
        for a in range(0, total, self.WINDOW_SLICE):
            b = min(total, a + self.WINDOW_SLICE)
            self.classify_bytes(arena, plan["win_off"][a:b], plan["win_len"][a:b], plan["max_len"], want_labels=False, logits=out[a:b])
        return out

    def window_fuse(self, plan, fuse="mean", logits=None, labels=None, want_labels=True, only_multi=False):
        """The windows' logits of a plan fused into one pair of logits per read (rd_window_fuse) on the current stream, which must see
        the windows' FINAL logits (sync_results()). only_multi: rows of reads with one window are left as they are."""
        n = plan["n"]
        if fuse not in N.WINDOW_FUSE:
            raise RuntimeError("classify_windows: fuse must be one of %s; got %r" % (", ".join(sorted(N.WINDOW_FUSE)), fuse))
        if logits is None:
            logits = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        if want_labels and labels is None:
            labels = torch.empty((n,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().rd_window_fuse(N.ptr(plan["win_logits"]), N.ptr(plan["win_first"]), n, N.WINDOW_FUSE[fuse], 1 if only_multi else 0,
                                           N.ptr(logits), N.ptr(labels if want_labels else None), N.stream_ptr(self.device)), "rd_window_fuse")
        return logits, (labels if want_labels else None)

    def classify_windows(self, arena, offsets, lens, max_len, stride=None, max_windows=32, fuse="mean", want_labels=True):
        """classify_bytes for reads of any length: a read longer than max_len is classified as W = min(max_windows, ceil((len - max_len) /
        stride) + 1) windows of max_len bases spread evenly from its start to its end (stride None = max_len), and the windows' logits
        are fused: "mean" = their fp32 mean in window order, "max" = the logits of the window with the largest rRNA margin. A read of at
        most max_len bases is its own window and its logits are classify_bytes' bit for bit (ribodetector_amd/windows.py has the rule
        in numpy). Returns (logits fp32[n, 2], labels uint8[n] | None, windows classified), FINAL: the call waits once on the host, for
        the number of windows, and runs the float64 pass of its windows before it fuses."""
        if fuse not in N.WINDOW_FUSE:
            raise RuntimeError("classify_windows: fuse must be one of %s; got %r" % (", ".join(sorted(N.WINDOW_FUSE)), fuse))
        plan = self.window_plan(lens, max_len, stride, max_windows)
        total = self.window_table(plan, offsets, lens)
        self.classify_window_table(arena, plan)
        self.sync_results()
        logits, labels = self.window_fuse(plan, fuse, want_labels=want_labels)
        return logits, labels, total

    def window_regions(self, arena_a, rec_start_a, lens_a, plan_a, arena_b=None, rec_start_b=None, lens_b=None, plan_b=None, rec_stride=1,
                       out_cap=None, out=None):
        """The rRNA regions of the reads of one or two plans as text lines (rd_region_format, csrc/rd_regions.hpp; regions.py has the rule
        and the line format) on the current stream, which must see the windows' FINAL logits (sync_results()). arena_x: the text that
        holds mate x's records; rec_start_x int64 on the device: record i starts at rec_start_x[i * rec_stride] and ends at the next entry;
        lens_x int32[n]; plan_x: a plan with "win_logits" (window_plan / window_table / classify_window_table). arena_b None = single-end.
        out_cap: the bytes reserved for the lines (None: regions.default_hint), or `out`, a uint8 device buffer to write into. Returns
        (out, info): info int64[8] on the device = {units, bytes, 0, fault, regions of mate 1, of mate 2, reads of mate 1 with a region,
        of mate 2}; fault 1 = the lines need info[1] bytes, more than out holds - call again with that much; fault 2 = the tables do not
        describe the text or the windows. Nothing is written on a fault."""
        from .. import regions as R
        n = plan_a["n"]
        paired = arena_b is not None
        mates = [(arena_a, rec_start_a, lens_a, plan_a)] + ([(arena_b, rec_start_b, lens_b, plan_b)] if paired else [])
        for text, rs, ln, plan in mates:
            if plan["n"] != n or plan["max_len"] != plan_a["max_len"] or "win_logits" not in plan:
                raise RuntimeError("window_regions: the plans must be classified plans of the same reads")
            if text.dtype != torch.uint8 or not text.is_cuda or rs.dtype != torch.int64 or not rs.is_cuda or not rs.is_contiguous() \
                    or rs.numel() < (n - 1) * rec_stride + 2 or ln.dtype != torch.int32 or not ln.is_cuda or not ln.is_contiguous() or ln.numel() < n:
                raise TypeError("window_regions: text uint8, rec_start int64 (n * rec_stride + 1 entries) and lens int32[n] CUDA tensors")
        total = sum(p["total"] for _, _, _, p in mates)
        lib = N.lib()
        if out is None:
            if out_cap is None:
                out_cap = R.default_hint(sum(int(t.numel()) for t, _, _, _ in mates[:1 if rec_stride == 2 else 2]), n, total, len(mates))
            out = torch.empty(((int(out_cap) + 255) // 256) * 256, dtype=torch.uint8, device=self.device)
            out_cap = int(out_cap)
        else:
            out_cap = int(out.numel()) if out_cap is None else min(int(out_cap), int(out.numel()))
        info = torch.empty(8, dtype=torch.int64, device=self.device)
        ws = torch.empty(max(int(lib.rd_region_workspace_bytes(n, total)), 256), dtype=torch.uint8, device=self.device)
        args = []
        for text, rs, ln, plan in mates:
            args += [N.ptr(text), int(text.numel()), N.ptr(rs), N.ptr(ln), N.ptr(plan["win_first"]), N.ptr(plan["win_logits"])]
        if not paired:
            args += [None, 0, None, None, None, None]
        with torch.cuda.device(self.device):
            N.check(lib.rd_region_format(*args, int(rec_stride), n, plan_a["max_len"], N.ptr(out), out_cap, N.ptr(info), N.ptr(ws), ws.numel(),
                                         N.stream_ptr(self.device)), "rd_region_format")
        return out, info              # (ws goes back to the pool of the stream it was taken from: reused behind this call only)

    # ---- reference-compatible call --------------------------------------------------------------------
    def forward2(self, x):
        """pack_seq=false entry of the reference (model/model.py:40-50 forward2 + last_pad_out_items :67-72): x is a padded
        Tensor [B, L, 4] of one-hot / all-zero rows; the BiLSTM runs over all L rows and the output row is the last non-zero
        one (row L-1 for an all-zero read). That is the 'padded' semantics of the kernels (the reference's CPU product uses the
        same function), so the rows are turned back into bases and classified with RD_SEM_PADDED and max_len = L."""
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != 4:
            raise TypeError("SeqModel.forward2 expects a padded Tensor [B, L, 4]; got %s" % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if self._handle is None:
            raise RuntimeError("SeqModel: call .to('cuda') before inference")
        dev = self.device
        data = x.to(dev, non_blocking=True)
        B, L = int(data.shape[0]), int(data.shape[1])
        if B == 0:
            return torch.empty((0, 2), dtype=torch.float32, device=dev)
        rs, mx = data.sum(2), data.max(2)
        ok = ((rs == 1) & (mx.values == 1)) | ((rs == 0) & (data.abs().sum(2) == 0))
        if not bool(ok.all()):
            raise ValueError("SeqModel.forward2: input rows must be one-hot (A,C,G,T) or all-zero")
        code = torch.where(rs == 1, mx.indices, torch.full_like(mx.indices, 4))
        arena = torch.tensor(list(b"ACGTN"), dtype=torch.uint8, device=dev)[code].reshape(-1)
        offsets = torch.arange(B, dtype=torch.int64, device=dev) * L
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        prev = self._semantics
        self.set_semantics("padded")
        try:
            logits, _ = self.classify_bytes(arena, offsets, lens, L, want_labels=False)
            self.sync_results()
        finally:
            self.set_semantics(prev)
        return logits

    def forward(self, x):
        """pack_seq=true (config.json): x is a PackedSequence of one-hot fp32 rows [sum T, 4] (what the reference collate
        builds, detect.py:681-685); returns logits fp32[B,2] in the original (unsorted) batch order, like forward1 +
        last_items(unsort=True). pack_seq=false: x is a padded Tensor -> forward2."""
        if not self.pack_seq:
            return self.forward2(x)
        if not isinstance(x, PackedSequence):
            raise TypeError("SeqModel.forward expects a PackedSequence (config pack_seq=true; build the model with pack_seq=false "
                            "for padded Tensor input, the reference's forward2); got %s" % type(x).__name__)
        if self._handle is None:
            raise RuntimeError("SeqModel: call .to('cuda') before inference")
        dev = self.device
        data = x.data.to(dev, non_blocking=True)
        if data.dim() != 2 or data.shape[1] != 4:
            raise ValueError("SeqModel.forward: PackedSequence.data must be [sum T, 4]")
        bs = x.batch_sizes.to(torch.int64).cpu()
        tmax, n, total = int(bs.numel()), int(bs[0]), int(data.shape[0])
        # rows must be one-hot or all-zero: that is the only input the reference encoder can produce
        rs, mx = data.sum(1), data.max(1)
        ok = ((rs == 1) & (mx.values == 1)) | ((rs == 0) & (data.abs().sum(1) == 0))
        if not bool(ok.all()):
            raise ValueError("SeqModel.forward: input rows must be one-hot (A,C,G,T) or all-zero")
        code = torch.where(rs == 1, mx.indices, torch.full_like(mx.indices, 4))
        ascii_ = torch.tensor(list(b"ACGTN"), dtype=torch.uint8, device=dev)[code]
        bs_d = bs.to(dev)
        t_of_row = torch.repeat_interleave(torch.arange(tmax, device=dev), bs_d, output_size=total)
        cum = torch.cumsum(bs_d, 0) - bs_d
        j_of_row = torch.arange(total, device=dev) - cum[t_of_row]
        sorted_idx = x.sorted_indices.to(dev) if x.sorted_indices is not None else torch.arange(n, device=dev)
        orig = sorted_idx[j_of_row]
        arena = torch.full((n, tmax), ord("N"), dtype=torch.uint8, device=dev)
        arena[orig, t_of_row] = ascii_
        len_sorted = (bs_d[None, :] > torch.arange(n, device=dev)[:, None]).sum(1)
        lens = torch.empty(n, dtype=torch.int32, device=dev)
        lens[sorted_idx] = len_sorted.to(torch.int32)
        offsets = torch.arange(n, dtype=torch.int64, device=dev) * tmax
        logits, _ = self.classify_bytes(arena.reshape(-1), offsets, lens, tmax, want_labels=False)
        self.sync_results()
        return logits

    __call__ = forward

    # ---- profiling hooks for bench.py ---------------------------------------------------------------
    def profile_enable(self, on=True):
        N.check(N.lib().rd_profile_enable(self._handle, 1 if on else 0), "rd_profile_enable")

    def profile_read(self):
        n, ms = C.c_int64(0), C.c_double(0)
        N.check(N.lib().rd_profile_read(self._handle, C.byref(n), C.byref(ms)), "rd_profile_read")
        return int(n.value), float(ms.value)

    def __str__(self):
        return "SeqModel(BiLSTM 4->128 x2, Linear 256->2) [HIP/gfx950]\nTrainable parameters: 137730"


def pair_fuse(logits1, logits2, ensure, counts=None):
    """Pair label logic of reference detect.py:616-663 on the device. Returns int8[n] in {0,1,-1};
    `counts` (uint64... stored as int64[3] tensor) is added to when given."""
    n = int(logits1.shape[0])
    out = torch.empty((n,), dtype=torch.int8, device=logits1.device)
    with torch.cuda.device(logits1.device):
        return _pair_fuse_launch(logits1, logits2, n, ensure, out, counts)


def _pair_fuse_launch(logits1, logits2, n, ensure, out, counts):
    N.check(N.lib().rd_pair_fuse(N.ptr(logits1), N.ptr(logits2), n, N.ENSURE_MODES[ensure], N.ptr(out), N.ptr(counts),
                                 N.stream_ptr(logits1.device)), "rd_pair_fuse")
    return out


def count_labels(labels, counts):
    """counts int64[3] device tensor (non-rRNA, rRNA, unclassified), added to (reference detect.py:485-486)."""
    with torch.cuda.device(labels.device):
        N.check(N.lib().rd_count_labels(N.ptr(labels), int(labels.numel()), N.ptr(counts), N.stream_ptr(labels.device)),
                "rd_count_labels")
    return counts
