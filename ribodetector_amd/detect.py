#!/usr/bin/env python3
"""`ribodetector` command line on MI355X - same flags, config.json lookup, log lines, output files and label rules as
the reference's GPU product (reference detect.py:34-809), with the per-batch host work (one-hot + pack_sequence in
DataLoader workers, detect.py:666-726) replaced by raw bytes -> HBM -> fused HIP kernels.

Flow per chunk (reference run_with_chunks, detect.py:326-523):
    FASTQ/FASTA chunk as one byte arena + offsets (data_loader/fastx_parser.py)
    -> pinned host buffer -> H2D on a copy stream (double buffered: chunk k+1 is parsed/copied while chunk k computes)
    -> rd_classify (R1 [, R2]) -> rd_pair_fuse / argmax -> labels D2H (1 B/read)
    -> records written by label in input order.
A run takes one of three layouts (Predictor._plan_ranks decides; under torchrun, WORLD_SIZE > 1, one process per GPU):
  * one rank: it reads, classifies and writes everything;
  * sharded parse - plain inputs, BGZF inputs (rank 0 indexes the members) and single-stream .gz inputs that the device decoder
    takes (every rank decodes its own compressed range, data_loader/gz_shard.py): every rank parses only its own share
    (record-aligned, mates cut at the same record index: data_loader/fastx_parser.plan_ranges), classifies it and writes its own
    part of every output file; the counters are all-reduced (RCCL) and every rank copies its part to its offset in the final file
    (rank order = input order);
  * label gather - the other gzip inputs (one DEFLATE stream decoded once per node into shared memory, or by every rank): every
    rank classifies a contiguous shard of each chunk, and rank 0 gathers the 1-byte labels - and the gzip members and report
    lines made of every shard - over RCCL and writes (ribodetector_amd/dist.py).
--interleaved (an extension): the pairs come from ONE FASTQ file whose records alternate mate 1, mate 2. Its chunks hold twice the
records; rd_pair_split (csrc/rd_pairs.hpp) turns a chunk's tables into the two mates' sequence tables and a table of the pairs and
checks the mates' ids, and from there on the run is the paired-end run (under several ranks: always the label gather).
--summary (an extension): every rank adds the QC counters of the units it classified to one int64 array on its GPU, chunk by chunk
(rd_summary_accumulate, summary.py); the arrays are summed after the last chunk and rank 0 writes them as JSON once the run has ended well.
--windows (an extension): a read longer than -l is classified over several windows of -l bases instead of its first -l bases alone. The
window table of a chunk is planned and written on the copy stream (rd_window_plan / rd_window_fill, csrc/rd_windows.hpp; windows.py has
the rule), rd_classify runs over it as it runs over a read table, and the post stream fuses the windows' final logits into one pair of
logits per read (rd_window_fuse); everything behind that - pair fusion, outputs, report, summary - sees reads.
--regions (an extension, with --windows): what the windows said before they were fused - the maximal runs of rRNA windows of every read,
as intervals in the read's bases, one text line each (regions.py has the rule; rd_region_format, csrc/rd_regions.hpp, formats a chunk's
lines on the post stream where the windows' final logits are). The lines travel like the per-read report's, as pieces of one more file.
BAM input (an extension): -i x.bam / x.ubam, in all three layouts of the inputs (one file, two files, --interleaved). The file's BGZF
members are inflated on the GPU and rd_bam_index (csrc/rd_bam_index.hpp; bam.py has the rule) frames the records and re-writes them as
FASTQ text, so the chunks are FASTQ chunks and the outputs FASTQ files. Device ingest only; one rank (check_bam), or - --bam_shard - the
sharded parse of the file's BGZF members: every rank frames its own share, which begins at a record start found by a search on the GPU
(data_loader/bam_shard.py; a cut that is no record start ends the run before any output is joined).
--bam_output (an extension, BAM input): the chunks also carry their records as they stand in the input (DeviceChunk.raw: rd_bam_raw_tab /
rd_bam_raw_gather, csrc/rd_bam_raw.hpp), and the output kernels select from THAT view (_select_chunk): every output is a BAM file - the
header of its input, the selected records byte for byte, BGZF members. Classification, report, summary and regions see the FASTQ view.
--read_groups (an extension, BAM input, with --summary): the chunks carry the same raw view, and every chunk's units are counted per
read group on the post stream (groups.py: rd_bam_tag_find / rd_bam_group_rows / rd_bam_group_accumulate); the summary gains "read_groups".
--split_groups (an extension, BAM input, one rank): every output file is a family of files, one per read group and one `unassigned`
(bam.split_paths); a chunk's records are partitioned by (class, group) key and deflated in ONE device call per mate (gz.DeviceGroupSelect:
rd_group_keys / rd_group_pack / rd_gz_compress_grouped), and the mate's writer appends every key's run to its file.
--bam_tags LIST (an extension, BAM input, FASTQ outputs): the chunks carry the raw view, and every chunk gets one more view, the TAGGED
text - its FASTQ text with the listed tags of every record behind the read name (bamtags.py: rd_bam_tag_splice, csrc/rd_bam_tagtext.hpp;
bam.tag_comment has the rule). It depends on the chunk alone, so it is made on the copy stream when the chunk is submitted; the output
kernels select from that view (_select_chunk), everything else sees the untagged FASTQ view. --bam_tag_floats: the tagged view is built
with the f and B:f values written in %g form (rd_bam_tag_splice_ex; bam.float_g has the rule) instead of skipped and counted.
--ubam_output (an extension, FASTQ / FASTA input, one rank, chunk text on the device): every output is an unaligned BAM file. A chunk's
raw view is MADE here - rd_bam_encode (ubam.py, csrc/rd_bam_encode.hpp; bam.from_fastq has the rule) on the copy stream when the chunk is
submitted - and from there on the run is --bam_output's: the output kernels select from DeviceChunk.raw, the files start with a header
(bam.UBAM_HEADER_TEXT, no references) and are BGZF. A record that cannot be a BAM record (a name of more than 254 bytes, a quality line
that is not as long as its sequence) ends the run like a mate mismatch: the chunks in front of it are written, then the ValueError.
--ubam_tags LIST (with --ubam_output): the records carry the listed tags that the comments of their header lines hold in SAM's text form
(rd_bam_encode_ex; bam.tags_from_comment has the rule) - the inverse of --bam_tags. The host then waits for each encode's verdict on the
copy stream: a chunk whose records need more than their buffer is encoded once more at the size the call reported. --ubam_tag_floats: the
f and B:f values of the listed tags become float32 tags instead of being left out (bam.float_from_text has the rule; csrc/rd_float_parse.hpp).
"""
import argparse
import functools
import math
import os
import threading
import time
import queue
from argparse import RawTextHelpFormatter
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import __version__
from . import _native as _native_mod
from . import bam as _bammod
from . import bamtags as _tagmod
from . import dist as rdist
from . import groups as _grpmod
from . import gz as _gzmod
from . import regions as _regmod
from . import summary as _summod
from . import ubam as _ubammod
from . import windows as _winmod
from .data_loader import device_reader as dr
from .data_loader import fastx_parser as fx
from .model import model as module_arch
from .parse_config import ConfigParser
from .ticket import RegionRepeat, Ticket

cd = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CHUNK_READS = 1 << 20      # records per chunk when --chunk_size is not given (reference: whole file in RAM)


class colors:
    HEADER = '\033[95m'
    OKBLUE = '\033[94m'
    OKCYAN = '\033[96m'
    OKGREEN = '\033[92m'
    OKYELLOW = '\033[33m'
    WARNING = '\033[93m'
    FAIL = '\033[91m'
    ENDC = '\033[0m'
    BOLD = '\033[1m'


def part_path(path, rank):
    """name of rank `rank`'s part of an output file; keeps a trailing 'gz' because the writer compresses by name
    (reference detect.py:738: read_file.endswith('gz')) - and a trailing '.bam' / '.ubam' (--bam_output under --bam_shard), by which
    the writer makes BGZF blocks"""
    if path.endswith('gz'):
        return '%s.part%d.gz' % (path[:-2].rstrip('.'), rank)
    for ext in ('.bam', '.ubam'):
        if path.endswith(ext):
            return '%s.part%d%s' % (path[:-len(ext)], rank, ext)
    return '%s.part%d' % (path, rank)


REPORT = (0, None)      # the --read_report among the (mate, label) output files: mate 1's writer appends it, it holds no label's records
REGIONS = (0, "regions")        # the --regions file, likewise
TEXT_FILES = (REPORT, REGIONS)  # files of text made on the device, not of a label's records


def _pinned(t):
    """a pinned host copy of a device tensor, queued on the current stream (read it once an event recorded behind it has passed)"""
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True)


def record_view(source, n, labels, e, interleaved=False, outs=2, pair_table=None, expand=None):
    """(text, record table, selecting labels) of mate e's records, as DeviceGzip.compress_selected and DeviceSelect.pack_selected take
    them - the one place that knows the three layouts. source: (text, record table) of this rank's n units; labels: the unit labels
    (None: the caller selects by key - gz.DeviceGroupSelect - and gets no labels, none are expanded).
      two input files: record k of mate e's source is unit k;
      interleaved, one output: pair k is records 2 k and 2 k + 1, so the table is every second entry - pair_table where the source
        has that table already (rd_pair_split wrote it), else a copy of the entries;
      interleaved, two outputs: mate e's records of the full table - expand(labels, e) labels record 2 k + e as pair k and the other
        mate's records RD_LABEL_SKIP, which no file selects (the run: DevicePairSplit.expand; the host: fx.expand_pair_labels)."""
    text, table = source
    if not interleaved:
        return text, table, labels
    if outs == 1:
        return text, table[0:2 * n + 1:2].contiguous() if pair_table is None else pair_table, labels
    return text, table, None if labels is None else expand(labels, e)


class Piece(NamedTuple):
    """Bytes that the GPU left for output files for one chunk (one piece per rank under the label gather). info: pinned copy of the
    int64[4] that the kernel which made buf wrote ([0] = gzip bytes, [1] = text bytes: gz.DeviceGzip / DeviceSelect / DeviceReport /
    DeviceGroupSelect), or None when all of buf counts (bytes gathered from the ranks); text: text or gzip members.
      A label piece is one run of bytes for ONE file, the key it stands under in Ticket.pieces. fault: pinned info whose [3] != 0 says
    that the chunk's record table did not describe its text to `what`; fallback: what the file gets when the bytes exceed buf (text
    that did not compress into the reserved half): None = the host writes the chunk's selected records.
      A grouped piece (--split_groups; key_tab is not None) holds the runs of ONE mate's family files from one grouped call: key_tab
    (pinned int64[K, 4]) says where - key s * (G + 1) + g is member g of the family of class labels[s] -, kinfo is the pinned int64[4]
    of rd_group_keys. It has no fallback: check_split_groups refuses the runs that would need one."""
    buf: torch.Tensor
    info: Optional[torch.Tensor]
    text: bool
    fault: Optional[torch.Tensor] = None
    what: str = "gzip"
    fallback: Optional["Piece"] = None
    key_tab: Optional[torch.Tensor] = None
    kinfo: Optional[torch.Tensor] = None
    labels: tuple = ()

    def size(self):
        """the bytes made, whether or not they fit buf; raises when the kernel found the chunk's tables wrong"""
        if self.key_tab is not None:
            if int(self.kinfo[0]):
                raise RuntimeError("device group keys: a label or a read-group row of the chunk is outside its range (flags %d)" % int(self.kinfo[0]))
            if int(self.info[3]):
                raise RuntimeError("device group %s: the chunk's keys or record table do not describe its text, or the output did not fit (fault %d)"
                                   % ("pack" if self.text else "gzip", int(self.info[3])))
        elif self.fault is not None and int(self.fault[3]):
            raise RuntimeError("device %s: the chunk's record table does not describe its text" % self.what)
        return int(self.buf.numel()) if self.info is None else int(self.info[1 if self.text else 0])

    def take(self):
        """(piece, bytes) that the files get: this piece, or its fallback when the bytes do not fit buf; (None, 0) = the host writes
        the chunk's selected records"""
        nb = self.size()
        if nb <= self.buf.numel() or self.key_tab is not None:
            return self, nb
        return (None, 0) if self.fallback is None else self.fallback.take()

    def runs(self, key, nb):
        """[(file key, offset in buf, bytes)] of the nb bytes that size() told, for a piece that stands under `key`"""
        if self.key_tab is None:
            return [(key, 0, nb)]
        tab = self.key_tab.numpy()
        G1 = len(tab) // len(self.labels)
        return [((key[0], self.labels[k // G1], k % G1), int(tab[k, 0]), int(tab[k, 1])) for k in np.flatnonzero(tab[:, 1])]


SPLIT = "groups"            # pieces[(mate, SPLIT)]: the grouped pieces of a mate's family files


class MateMismatch(RuntimeError):
    """--interleaved: two consecutive records whose ids are not those of mates (the chunks in front of them have been written)"""


class UbamRecordError(ValueError):
    """--ubam_output: a record that cannot be a BAM record (the chunks in front of its chunk have been written)"""


class _MateWriter:
    """The writer thread of one mate: the records of that mate's output files in input order (mate 1's: and the per-read report).
    Two sets of pinned staging buffers: the bytes an item's files get from the GPU (gzip members / packed records / report text) are
    fetched for item k+1 while item k is being written. The fetch is a kernel on this thread's stream (C ABI rd_copy_bytes), not a
    DMA copy - an SDMA queue is shared in order with copies that wait for kernels."""

    def __init__(self, pred, e, files, errors):
        self.pred, self.e, self.files, self.errors = pred, e, files, errors     # files: [((mate, label), handle)] of mate e in file order
        self.keys, self.handles = self._file_index(e, files)
        self.q = queue.Queue(maxsize=2)      # items (chunk of this mate, labels, Ticket.pieces); None ends
        self.stream, self.stages = _gzmod.acquire_stream(pred.device), [[], []]
        self.thread = pred._spawn(self._run)

    def _run(self):
        item = ()
        try:
            torch.cuda.set_device(self.pred.device)          # (the current device is per thread)
            pending, k = None, 0
            while True:
                try:
                    item = self.q.get() if pending is None else self.q.get_nowait()
                except queue.Empty:         # nothing to prefetch: write what is in hand, then wait
                    self._complete(*pending)
                    pending = None
                    continue
                if item is not None:
                    nxt, k = (item, self._issue(item, k)), k ^ 1
                if pending is not None:
                    self._complete(*pending)
                if item is None:
                    return
                pending = nxt
        except BaseException as ex:
            self.errors.append(ex)
            while item is not None:          # keep draining so that the producer never blocks
                item = self.q.get()
        finally:
            self.pred.thread_cpu_s["writer:%d" % self.e] = round(time.thread_time(), 4)

    @staticmethod
    def _file_index(e, files):
        """(the keys under which an item's pieces for mate e's files stand, in job order; {file key: handle}). The family members
        (keys of three) share the grouped pieces under (e, SPLIT); every other file has its own key."""
        own = [key for key, _ in files if len(key) != 3]
        return ([(e, SPLIT)] if len(own) < len(files) else []) + own, dict(files)

    def _issue(self, item, k):
        """queue the D2H of everything the item's files take from the GPU into stage set k; returns the writes - those of any one file
        in input order -, as (event to wait for or None, write)"""
        chunk, labels, pieces = item
        jobs, slot = [], 0
        for key in self.keys:
            # (a file without a piece: the host writes the records of its label; family members only ever get what the grouped pieces hold)
            for piece in pieces.get(key) or (() if key[1] == SPLIT else (None,)):
                p, nb = (None, 0) if piece is None else piece.take()
                if p is None:           # nothing from the GPU, or too much for its buffer: the host writes the records of this label
                    jobs.append((None, functools.partial(self.handles[key].write_selected, chunk, labels, key[1])))
                    continue
                if p.key_tab is not None:
                    self.pred._split_counted(self.e, p.labels, p.key_tab.numpy()[:, 2])
                if nb:
                    buf, done = p.buf, None
                    if buf.is_cuda:
                        (buf, done), slot = self._fetch(k, slot, buf, nb), slot + 1
                    for fkey, off, n in p.runs(key, nb):
                        fh = self.handles[fkey]
                        jobs.append((done, functools.partial(fh.write_text if p.text else fh.write_members, buf.data_ptr() + off, n)))
        return jobs

    def _fetch(self, k, slot, src, nb):
        """the first nb bytes of device buffer src -> pinned staging buffer `slot` of set k; returns (staging buffer, event)"""
        st = self.stages[k]
        if slot == len(st):
            st.append(None)
        if st[slot] is None or st[slot].numel() < nb:
            st[slot] = None
            st[slot] = torch.empty(max(nb, 1 << 22) * 5 // 4, dtype=torch.uint8, pin_memory=True)
        _native_mod.copy_bytes(st[slot], src, nb, self.stream)
        done = _native_mod.new_event()
        done.record(self.stream)
        return st[slot], done

    @staticmethod
    def _complete(item, jobs):
        for done, write in jobs:
            if done is not None:
                _native_mod.wait_event(done)    # (sleeping in the driver: stream.synchronize() would spin a core)
            write()
        if item[0].release is not None:   # a shared-memory slot: free for the next chunk once its text is written
            item[0].release()


class Predictor:
    """Main class of predictor for rRNA, non-rRNA sequences (interface of reference detect.py:34-43)."""

    GZ_RING = 6          # device gzip: sets of output buffers in flight (submitted x2, queued x2, being written, + 1)

    def __init__(self, config, args, log_level=None):
        self.config = config
        self.args = args
        # under torchrun only rank 0 owns the log file (the other ranks log to the console only)
        self.logger = config.get_logger('predict', 1, self.args.log if int(os.environ.get('RANK', '0')) == 0 else None)
        log_level = log_level or os.environ.get('RD_LOG_LEVEL')     # (benchmarks call main() with "WARNING": no per-chunk lines)
        import logging
        self.logger.setLevel(getattr(logging, str(log_level).upper()) if log_level else logging.NOTSET)
        self.chunk_size = self.args.chunk_size
        self.thread_cpu_s = {}
        self.rank, self.world, self.local_rank = 0, 1, 0
        self.multi = False                       # collectives in use: several ranks (or one rank under RD_FORCE_DIST=1, dist.py)
        self._arenas = []                        # shared-memory chunk arenas of this rank (rank 0, gzip input, several ranks)
        self._part_files = []                    # this rank's part files of a sharded-parse run (removed if the run fails)
        self.sharded_parse = False               # the sharded-parse layout: every rank parses its own share of the input (_plan_ranks)
        self._shared = None                      # gzip input, several ranks of one node: one decode per node (decided once per run)
        self._chunk_reads = None
        self._use_device = None                  # does the text of the inputs stay on the device? decided once per run
        # the options that a hand-built Namespace may lack (tests, API users) are read here, once; everything below uses the attributes
        self.report_path, self.summary_path, self.regions_path, self.bam_tags_arg = (
            getattr(args, k, None) for k in ('read_report', 'summary', 'regions', 'bam_tags'))
        self._report = None                      # --read_report: gz.DeviceReport (run_with_chunks)
        self.interleaved = bool(getattr(args, 'interleaved', False))     # paired-end reads from ONE interleaved FASTQ file
        self.mate_check = not getattr(args, 'no_mate_check', False)
        self.bam_output = bool(getattr(args, 'bam_output', False))       # BAM outputs: the selected records as they stand in the input
        self.ubam_output = bool(getattr(args, 'ubam_output', False))     # BAM outputs of FASTQ / FASTA input: the records encoded on the device
        self.bam_files = self.bam_output or self.ubam_output             # every output file is a BAM file, whichever way its records are made
        self._ubam = None                        # ... ubam.DeviceUbam, one per input file (run_with_chunks)
        # --ubam_tags LIST: the names whose tags the records take from their header lines' comments (None: no tags)
        self.ubam_tag_floats = bool(getattr(args, 'ubam_tag_floats', False))      # ... with the f and B:f values as float32 tags
        self.ubam_tags = check_ubam_tags(getattr(args, 'ubam_tags', None), self.ubam_output, self.ubam_tag_floats)
        self.read_groups = bool(getattr(args, 'read_groups', False))     # --summary gains the counters per BAM read group
        self.split_groups = bool(getattr(args, 'split_groups', False))   # every output file becomes a family: a file per BAM read group
        self._split = self._split_ids = None     # ... gz.DeviceGroupSelect (run_with_chunks), the declared ids in row order (detect)
        self.bam_shard = bool(getattr(args, 'bam_shard', False))         # BAM input under several ranks: the sharded parse (data_loader/bam_shard.py)
        self._groups = None                      # ... groups.DeviceGroups (run_with_chunks)
        self.bam_tags = _tagmod.parse_list(self.bam_tags_arg) if self.bam_tags_arg is not None else None     # ... the listed names (2 bytes each)
        self.bam_tag_floats = bool(getattr(args, 'bam_tag_floats', False))      # ... with the f and B:f values as %g text
        self._tags = None                        # ... bamtags.DeviceBamTags, one per input file (run_with_chunks)
        self._pairs = None                      # --interleaved: gz.DevicePairSplit (run_with_chunks)
        self._summary = None                     # --summary: summary.DeviceSummary (run_with_chunks)
        self._windows = None                     # --windows: {"stride", "max_per_read", "fuse"} (stride None = -l); detect() sets it
        self._win_classified = [0, 0]            # windows this rank classified, per mate
        self._regions = False                    # --regions: a piece of region lines per chunk (run_with_chunks)
        self._reg_counts = [0, 0, 0, 0]          # this rank's regions of mate 1 / 2 and reads of mate 1 / 2 with a region
        self.regions_repeats = 0                 # chunks whose lines did not fit the reserved bytes and were formatted again
        self._install_cleanup()

    @property
    def gathers_labels(self):
        """the label-gather layout (module docstring): several ranks classify shards of one decode, and rank 0 gathers and writes"""
        return not self.sharded_parse and self.multi

    # ---- cleanup ------------------------------------------------------------------------------------
    def cleanup(self):
        """what a run must not leave behind, whichever way it ends: the shared-memory chunk slots (they are RAM) and this rank's
        '<out>.partN' / '<out>.joining' files"""
        self._close_arenas()
        for f in self._part_files:
            try:
                os.remove(f)
            except OSError:
                pass
        self._part_files = []

    def _install_cleanup(self):
        """atexit + SIGTERM: when ANOTHER rank fails, torch.distributed.run sends this one SIGTERM - the default action would end the
        process without running any Python, and rank 0's slot files would stay in /dev/shm until the node reboots"""
        import atexit
        import signal
        import weakref
        ref = weakref.ref(self)

        def run():
            me = ref()
            if me is not None:
                me.cleanup()
        atexit.register(run)
        if threading.current_thread() is threading.main_thread():
            prev = signal.getsignal(signal.SIGTERM)

            def on_term(signum, frame):
                run()
                signal.signal(signal.SIGTERM, prev if callable(prev) or prev in (signal.SIG_DFL, signal.SIG_IGN) else signal.SIG_DFL)
                os.kill(os.getpid(), signal.SIGTERM)
            try:
                signal.signal(signal.SIGTERM, on_term)
            except (ValueError, OSError):
                pass

    # ---- model -------------------------------------------------------------------------------------
    def get_state_dict(self):
        """'recall' weights iff --ensure norrna, else 'mcc' (reference detect.py:45-82)."""
        self.len = self.args.len
        if self.len < 40:
            self.logger.info('The accuracy will drop with reads shorter than 40.')
        model_file_ext = 'recall' if self.args.ensure == 'norrna' else 'mcc'
        self.state_key = model_file_ext
        self.state_file = self.config.state_file(model_file_ext)
        self.logger.info('Using high {} model'.format(model_file_ext.upper()))
        self.logger.info('Log file: {}'.format(self.args.log))

    def kernel_config(self):
        """the `kernel` block of config.json (specific to this build), validated before anything touches the GPU"""
        kcfg = dict(self.config.config.get('kernel', {}))
        variant = kcfg.get('variant', 'auto')
        if variant not in ('auto', 'mfma_f32', 'simple', 'mfma_f16x3_t32'):
            raise RuntimeError("config.json kernel.variant must be one of auto, mfma_f16x3_t32, mfma_f32, simple; got %r" % (variant,))
        sem = getattr(self.args, 'semantics', None) or kcfg.get('semantics', 'gpu')
        if sem not in ('gpu', 'cpu', 'packed', 'padded'):
            raise RuntimeError("config.json kernel.semantics must be gpu or cpu; got %r" % (sem,))
        refine = float(kcfg.get('refine', module_arch.SeqModel.REFINE_DEFAULT))
        if not 0.0 <= refine <= 1.0:
            raise RuntimeError("config.json kernel.refine must be in [0, 1]; got %r" % (refine,))
        pk = kcfg.get('prefix_k', None)           # prefix-state table: absent = the model's default (RD_PREFIX_K or "auto")
        if pk is not None and pk != 'auto' and not (isinstance(pk, int) and (pk == 0 or 4 <= pk <= 13)):
            raise RuntimeError("config.json kernel.prefix_k must be \"auto\", 0 or an integer in [4, 13]; got %r" % (pk,))
        gz = os.environ.get("RD_DEVICE_GZIP") or kcfg.get("gzip", "device")     # who deflates .gz outputs: the GPU (BGZF members) or the host
        gz = {"1": "device", "0": "host"}.get(gz, gz)
        if gz not in ("device", "host"):
            raise RuntimeError("config.json kernel.gzip must be \"device\" or \"host\"; got %r" % (gz,))
        return {"variant": variant, "semantics": sem, "refine": refine, "prefix_k": pk, "gzip": gz}

    def prefix_k_for_input(self):
        """k of the prefix-state table that pays off for THIS run: a row saves k steps per read, level k costs 4^k one-step
        workgroup slots to build (measured on MI355X, tools/time_setup.py: k = 8 / 10 / 11 / 12 take 0.4 / 1.7 / 6.3 / 22 ms with
        their allocation; one read-step is worth 0.3 ns), so k+1 beats k from about 3 * 4^k reads on. The read count is estimated
        from the input sizes (gzip: x4.5) and -l; under torchrun every rank sees its share."""
        from .data_loader import fastx_parser as fx
        n = 0.0
        for path in self.args.input or []:
            try:
                size, gz = fx.file_info(path)
                fa = fx.get_seq_format(path).startswith("fa")
            except Exception:      # the run itself reports unreadable inputs
                continue
            n += size * (4.5 if gz else 1.0) / ((1 if fa else 2) * max(self.args.len, 30) + 30)
        n /= max(1, int(os.environ.get("WORLD_SIZE", "1")))
        return 8 if n < 2e6 else 10 if n < 14e6 else 11 if n < 49e6 else 12

    def load_model(self):
        """Load the model onto the GPU (reference detect.py:84-119). Raises RuntimeError without a visible device."""
        kcfg = self.kernel_config()
        if self.args.deviceid is not None:
            os.environ["HIP_VISIBLE_DEVICES"] = self.args.deviceid
            os.environ["CUDA_VISIBLE_DEVICES"] = self.args.deviceid
        self.rank, self.world, self.local_rank = rdist.init_from_env()
        self.multi = rdist.active()
        self.get_state_dict()
        model = self.config.init_obj('arch', module_arch)
        if not torch.cuda.is_available():
            self.logger.error('{}No visible GPU devices!{} This build runs the HIP kernels only; the CPU product of the '
                              'reference is ribodetector_cpu'.format(colors.FAIL, colors.ENDC))
            raise RuntimeError("Set HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES or use CPU inference.")
        if self.multi:                           # one process per GPU; RD_LOCAL_DEVICE pins a rank elsewhere (ranks sharing a GPU)
            self.device = torch.device('cuda', int(os.environ.get('RD_LOCAL_DEVICE', self.local_rank)))
            torch.cuda.set_device(self.device)
        else:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.has_cuda = True
        if self.multi and self.world > 1:        # (round 6) a rank's threads stay on its share of the CPUs next to its GPU; RD_PIN=0: off
            lw = int(os.environ.get("LOCAL_WORLD_SIZE", self.world))
            self.pinned_cpus, how = rdist.pin_rank_cpus(self.device.index, self.local_rank, lw)
            if self.pinned_cpus is not None:
                self.logger.info('Rank {} runs on CPUs {} ({})'.format(self.rank, ",".join(str(c) for c in self.pinned_cpus), how))
        model.load_state_dict(self.config.load_state_dict(self.state_key))
        self.logger.info('Model using {} for read length {}{}{}{} loaded'.format(
            self.device, colors.BOLD, colors.OKCYAN, self.len, colors.ENDC))
        if kcfg["prefix_k"] is not None:
            model.set_prefix_table(kcfg["prefix_k"])     # recorded now, built by .to()
        elif "RD_PREFIX_K" not in os.environ:
            model.set_prefix_table("auto", cap=self.prefix_k_for_input())
        self.model = model.to(self.device)
        self.model.set_variant(kcfg["variant"])
        self.model.set_semantics(kcfg["semantics"])
        # margin band of the float64 re-evaluation (config.json kernel.refine; 0 = off; default 2.5e-4), as the deferred pass of the
        # C ABI (rd_set_refine_async): the recurrence kernel's epilogue records the reads inside the band, and submit_chunk's
        # post-pass evaluates them (rd_sync_results on the post stream) beside the next chunk's recurrences.
        self.refine_band = kcfg["refine"]
        self.gzip_on_device = kcfg["gzip"] == "device"
        self.model.set_refine(self.refine_band)
        self.model.set_refine_async(16 if self.refine_band > 0 else 0)
        self.model.eval()

    # ---- classification of one chunk ------------------------------------------------------------------
    def _to_device(self, chunk, lo, hi, stream):
        """async H2D of records [lo, hi) of a chunk: only the bytes spanning those reads travel. The native reader parsed
        straight into pinned buffers, so there is no staging copy."""
        b0 = int(chunk.rec_start[lo])
        b1 = int(chunk.rec_start[hi])
        tbuf, toff, tlen = chunk.tensors[:3]
        with torch.cuda.stream(stream):
            arena = tbuf[b0:b1].to(self.device, non_blocking=True) if b1 > b0 else torch.zeros(1, dtype=torch.uint8, device=self.device)
            off = toff[lo:hi].to(self.device, non_blocking=True) - b0
            ln = tlen[lo:hi].to(self.device, non_blocking=True)
        return arena, off, ln

    def _fastq_view(self, chunks, dev_in, e, lo, hi, pairs=None):
        """the FASTQ view of mate e's units [lo, hi) of a chunk as a source of record_view: ((text, int64 record starts) on the device,
        table of the pairs or None). Interleaved: one text for both mates, and rd_pair_split left the table of its pairs beside it."""
        if pairs is not None:
            return (pairs["text"], pairs["rec_start"]), pairs["pair_start"]
        chunk = chunks[e]
        if isinstance(chunk, dr.DeviceChunk):
            return (chunk.dev[0], chunk.dev[3]), None
        return (dev_in[e][0], chunk.tensors[3][lo:hi + 1].to(self.device, non_blocking=True) - int(chunk.rec_start[lo])), None

    def _split_pairs(self, tk, chunk, lo, hi, on_dev, ring):
        """--interleaved: pairs [lo, hi) of a chunk of 2n records as two mates. The split runs once the chunk's tables are on the device
        (a device chunk: behind its `ready` event; a host chunk: after the H2D of records [2 lo, 2 hi)). Returns (dev_in of the two
        mates over the ONE text, pairs): pairs = the text with its record table and its pair table, for the outputs and the report, and
        the pinned verdict of the mate check, which the ticket's "pairs" check reads after the event collect_chunk waits for anyway."""
        cs, cur = self._copy_stream, torch.cuda.current_stream(self.device)
        if on_dev:
            cur.wait_event(chunk.ready)
            text, so, sl, rs = chunk.dev
        else:
            text, so, sl = self._to_device(chunk, 2 * lo, 2 * hi, cs)
            with torch.cuda.stream(cs):
                rs = chunk.tensors[3][2 * lo:2 * hi + 1].to(self.device, non_blocking=True) - int(chunk.rec_start[2 * lo])
            cur.wait_stream(cs)
        pair_start, m1, m2, info = self._pairs.split(text, rs, so, sl, hi - lo, check_ids=self.mate_check, slot=ring)
        pairs = {"text": text, "rec_start": rs, "pair_start": pair_start, "info": _pinned(info), "lo": lo,
                 "first_record": self._chunk_first_record, "keep": (so, sl)}
        tk.checks["pairs"] = functools.partial(self._check_pairs, chunk, pairs)
        return [(text,) + m1, (text,) + m2], pairs

    def _read_work(self, seq_len):
        """recurrence steps per read, for the shard bounds of the label gather: min(len, -l), times the read's windows under --windows"""
        ln = np.asarray(seq_len, dtype=np.int64)
        work = np.minimum(ln, self.len)
        if self._windows is not None:
            work = work * _winmod.counts(ln, self.len, self._windows["stride"] or self.len, self._windows["max_per_read"])
        return work

    def _plan_windows(self, tk, chunks, lo, hi, on_dev, ring):
        """--windows: the chunk's tables reach the device and the window table of every mate is planned and written on the COPY stream
        (behind the chunk's `ready` event or its H2D - not behind the recurrences of the chunk before, which fill the main stream); the
        host waits there, once, for the numbers of windows, which size the tables and the classify calls. The main stream then waits
        for the copy stream as it does without the flag. Returns (dev_in, pairs, one plan per mate)."""
        cs, cur = self._copy_stream, torch.cuda.current_stream(self.device)
        w, pairs = self._windows, None
        with torch.cuda.stream(cs):
            if self.interleaved:
                dev_in, pairs = self._split_pairs(tk, chunks[0], lo, hi, on_dev, ring)
            elif on_dev:
                dev_in = [c.dev[:3] for c in chunks]
                for c in chunks:
                    cs.wait_event(c.ready)
            else:
                dev_in = [self._to_device(c, lo, hi, cs) for c in chunks]
            plans = [self.model.window_plan(l, self.len, w["stride"], w["max_per_read"]) for _, _, l in dev_in]
            for e, (p, (_, o, l)) in enumerate(zip(plans, dev_in)):
                self._win_classified[e] += self.model.window_table(p, o, l)
        cur.wait_stream(cs)
        return dev_in, pairs, plans

    def _check_pairs(self, chunk, pairs):
        """the verdict of rd_pair_split on this rank's pairs of a chunk, once the event behind it has passed"""
        info = pairs["info"]
        if int(info[3]):
            raise RuntimeError("device pair split: the chunk's record table does not describe its text")
        k = int(info[1])
        if k < 0:
            return
        k += pairs["lo"]                             # pair k of the chunk: its records 2 k and 2 k + 1
        if isinstance(chunk, dr.DeviceChunk):        # (a failing run may wait for the three table entries and the two header lines)
            rs = chunk.dev[3][2 * k:2 * k + 3].cpu().numpy()
            buf, rs = chunk.dev[0][int(rs[0]):int(rs[2])].cpu().numpy(), rs - int(rs[0])
        else:
            buf, rs = chunk.buf, chunk.rec_start[2 * k:2 * k + 3]
        ids = [fx.record_id(buf, int(rs[i]), int(rs[i + 1])).decode("latin-1") for i in (0, 1)]
        first = pairs["first_record"] + 2 * k + 1
        raise MateMismatch("interleaved input: records {} and {} are not mates (ids '{}' and '{}'): a record is missing or the file is "
                           "not interleaved; --no_mate_check turns this check off".format(first, first + 1, ids[0], ids[1]))

    def submit_chunk(self, chunks, seq=None):
        """Enqueue one chunk: H2D on the copy stream, kernels on the compute stream, D2H of the labels into pinned memory.
        Nothing here waits for the GPU, so the next chunk's H2D overlaps this chunk's kernels. seq: the chunk's number in the run
        (None: the one behind the last chunk's); it picks the ring slot of every buffer that the pair split, the selection, the report
        and the regions write for this chunk. Returns a Ticket for collect_chunk()."""
        seq = self._chunk_seq if seq is None else seq
        self._chunk_seq, ring = seq + 1, seq % self.GZ_RING
        n = fx.interleaved_pairs(chunks[0]) if self.interleaved else len(chunks[0].seq_len)
        bounds = None
        if self.gathers_labels:                     # equal bases (= recurrence steps) per rank, not equal read counts
            if self.interleaved:
                work = self._read_work(chunks[0].seq_len[:2 * n]).reshape(n, 2).sum(1)
            else:
                work = sum(self._read_work(c.seq_len) for c in chunks)
            bounds = rdist.shard_bounds(n, self.world, work)
        lo, hi = (0, n) if bounds is None else (bounds[self.rank], bounds[self.rank + 1])
        cs = self._copy_stream
        cur = torch.cuda.current_stream(self.device)
        on_dev = isinstance(chunks[0], dr.DeviceChunk)      # text and index already in HBM (data_loader/device_reader.py): nothing to copy
        tk = Ticket(n, bounds, chunks[0])
        totals = [t for c in chunks for t in (c.total, c.raw_total) if t is not None] if on_dev else ()
        if totals:                                  # the bytes rd_fastq_gather made of the chunk's views, pinned behind `ready`
            tk.checks["totals"] = functools.partial(self._check_totals, totals)
        pairs = plans = None
        if self._windows is not None:
            dev_in, pairs, plans = self._plan_windows(tk, chunks, lo, hi, on_dev, ring)
        elif self.interleaved:
            dev_in, pairs = self._split_pairs(tk, chunks[0], lo, hi, on_dev, ring)
        elif on_dev:
            dev_in = [c.dev[:3] for c in chunks]
            for c in chunks:
                cur.wait_event(c.ready)
        else:
            dev_in = [self._to_device(c, lo, hi, cs) for c in chunks]
            cur.wait_stream(cs)
        tagged = self._tag_chunks(chunks, on_dev) if self._tags is not None else None      # --bam_tags: the view the outputs select from
        encoded = self._ubam_chunks(tk, chunks, on_dev) if self._ubam is not None else None   # --ubam_output: the raw view, made here
        if plans is None:
            outs = [self.model.classify_bytes(a, o, l, self.len, want_labels=not self.is_paired) for a, o, l in dev_in]
        else:                                       # (the window tables: the reads' own entries where nothing is longer than -l)
            for (a, _, _), p in zip(dev_in, plans):
                self.model.classify_window_table(a, p)
        main_done = torch.cuda.Event()
        main_done.record(cur)
        # post-pass on its own stream: it overlaps the recurrences of the next chunk (the float64 refine pass has the latency of
        # one read with most of the GPU idle)
        post = self._post_stream
        with torch.cuda.stream(post):
            post.wait_event(main_done)
            if encoded is not None:
                post.wait_event(encoded)
            self.model.sync_results()                # the reads inside the noise band, in float64 (current stream = post)
            if plans is not None:                    # the windows' logits are final: one pair of logits per read
                outs = [self.model.window_fuse(p, self._windows["fuse"], want_labels=not self.is_paired) for p in plans]
            if self.is_paired and self.args.ensure == 'none' and self.refine_band > 0:
                # pair label = argmax of the SUMMED logits (reference detect.py:657): also the reads whose PAIR margin is inside the
                # band - only both mates' logits together say which, so this mode keeps the scan form of the pass (rd_refine)
                for k, (a, o, l) in enumerate(dev_in):
                    self.model.refine(a, o, l, self.len, outs[k][0], outs[k][1], outs[1 - k][0], thresh=self.refine_band)
                    if plans is not None:            # the pass read the read-level tables: a read of several windows gets its fused logits back
                        self.model.window_fuse(plans[k], self._windows["fuse"], logits=outs[k][0], labels=outs[k][1],
                                               want_labels=outs[k][1] is not None, only_multi=True)
            labels = module_arch.pair_fuse(outs[0][0], outs[1][0], self.args.ensure) if self.is_paired else outs[0][1].view(torch.int8)
            tk.labels, tk.host = labels, None if self.gathers_labels else _pinned(labels)
            rows1 = self._group_rows(chunks[0]) if self._split is not None else None     # mate 1's rows, once: the split and --read_groups
            tk.pieces = self._select_chunk(chunks, dev_in, labels, lo, hi, on_dev, ring, pairs, tagged, rows1)
            if self._report is not None:
                tk.pieces[REPORT] = self._report_chunk(chunks, dev_in, outs, labels, lo, hi, ring, pairs)
            if self._regions:
                piece, reg = self._regions_chunk(chunks, dev_in, plans, lo, hi, pairs, ring=ring)
                tk.pieces[REGIONS] = [piece]
                tk.checks["regions"] = functools.partial(self._finish_regions, tk.pieces, reg)
            if self._summary is not None:          # --summary: this rank's units of the chunk, counted where they are (rd_summary_accumulate)
                info = _pinned(self._summary.add(dev_in[0], outs[0][0], dev_in[1] if self.is_paired else None,
                                                 outs[1][0] if self.is_paired else None, labels.view(torch.int8)))
                tk.checks["summary"] = functools.partial(self._check_counted, "summary: the chunk's sequence tables or labels", info)
            if self._groups is not None:            # --read_groups: the same units per read group, over the chunks' raw records
                info = _pinned(self._groups.add(chunks, labels.view(torch.int8), self.interleaved, rows_a=rows1))
                tk.checks["groups"] = functools.partial(self._check_counted, "read groups: the chunk's labels or group rows", info)
            if self.gathers_labels:                 # label gather (1 B per read) queued behind the kernels, collected later
                _, tk.finish = rdist.gather_labels(labels, n, dst=0, bounds=bounds, async_op=True)
            tk.done = _native_mod.new_event()
            tk.done.record(post)
        # what the ticket only keeps alive: the tensors of dev_in (of pairs, of the tagged views; --read_groups: the raw views) were
        # allocated on the copy stream and must not return to that stream's pool while other streams read them - and the deferred
        # float64 pass reads the bases until the post-pass has run
        tk.keep = (dev_in, outs, plans, pairs, tagged, [c.raw for c in chunks] if self._groups is not None or self._split is not None or self._ubam is not None else None)
        return tk

    def _tag_chunks(self, chunks, on_dev):
        """--bam_tags: [(tagged text, its record table)] of every input's chunk (bamtags.DeviceBamTags.splice), made on the COPY stream
        behind the chunk's `ready` event - not behind the recurrences of the chunk before, which fill the main stream. The host waits
        there for the call's verdict and sizes (a chunk that did not fit its hint is spliced again), as it waits for the window plans."""
        if not on_dev:
            raise RuntimeError("--bam_tags: the chunk's text is not on the device (BAM input is device ingest only)")
        out = []
        with torch.cuda.stream(self._copy_stream):
            for c, tg in zip(chunks, self._tags):
                self._copy_stream.wait_event(c.ready)
                _native_mod.wait_event(c.ready)
                self._check_totals((c.total, c.raw_total))     # (here already: the splice reads the views before collect_chunk runs)
                text, out_start, _ = tg.splice(c)
                out.append((text, out_start))
        return out

    def _ubam_chunks(self, tk, chunks, on_dev):
        """--ubam_output: every input's chunk gets its raw view - its records as BAM records (ubam.DeviceUbam.encode) - on the COPY
        stream behind the chunk's `ready` event, where the tag splice runs; like it, the encode needs no labels. Nothing waits: the
        bound of the raw bytes is linear in the text. Returns the event behind the calls; the ticket's "ubam" check reads their verdicts.
        --ubam_tags: DeviceUbam.encode waits for each call's verdict there (a second call at the exact size) and hands its info over on the host."""
        if not on_dev:
            raise RuntimeError("--ubam_output: the chunk's text is not on the device")
        infos, cs = [], self._copy_stream
        with torch.cuda.stream(cs):
            for f, (c, ub) in enumerate(zip(chunks, self._ubam)):
                cs.wait_event(c.ready)
                raw, raw_start, info = ub.encode(c, _bammod.INTERLEAVED if self.interleaved else f, 2 if self.is_paired else 1)
                c.raw = (raw, raw_start)
                infos.append(info if self.ubam_tags else _pinned(info))      # (--ubam_tags: the host has waited for the verdict already)
            done = torch.cuda.Event()
            done.record(cs)
        first, self._ubam_seen = self._ubam_seen, self._ubam_seen + len(chunks[0].seq_len)
        tk.checks["ubam"] = functools.partial(self._check_ubam, infos, first)
        return done

    def _check_ubam(self, infos, first):
        """the verdicts of rd_bam_encode on a chunk, once the event behind them has passed: the counters are added up; a record that
        cannot be a BAM record ends the run - first = the index of the chunk's first record in its file"""
        worst = None
        for ub, info in zip(self._ubam, infos):
            long_name, mismatch = ub.add(info)
            for idx, text in ((long_name, _bammod.UBAM_NAME_ERROR), (mismatch, _bammod.UBAM_LENGTH_ERROR)):
                if idx >= 0 and (worst is None or idx < worst[0]):
                    worst = (idx, text)
        if worst is not None:
            raise UbamRecordError(worst[1] % (first + worst[0]))

    def _group_rows(self, chunk):
        """the read-group rows of every raw record of mate 1's chunk (rd_bam_tag_find / rd_bam_group_rows over DeviceChunk.raw)"""
        if chunk.raw is None:
            raise RuntimeError("--split_groups: the chunk carries no raw records (BAM input is device ingest only)")
        raw, rs = chunk.raw
        return self._split_dict.rows(raw, *_grpmod.tag_find(raw, rs, int(rs.numel()) - 1, _grpmod.TAG))

    def _output_view(self, chunks, dev_in, labels, e, lo, hi, ring, pairs, tagged):
        """(text, record table, selecting labels) of mate e's records for the output files - the one place that chooses their source:
        the records as they stand in the input under --bam_output, or as rd_bam_encode made them under --ubam_output
        (DeviceChunk.raw), else the text with the tags behind the read names under --bam_tags, else the FASTQ view; record_view
        knows the layouts. labels None (--split_groups selects by key): no selecting labels, none expanded."""
        f, pair_table = e if pairs is None else 0, None
        if self.bam_files:
            source = chunks[f].raw
        elif tagged is not None:
            source = tagged[f]
        else:
            source, pair_table = self._fastq_view(chunks, dev_in, e, lo, hi, pairs)
        return record_view(source, hi - lo, labels, e, pairs is not None, len(self.output), pair_table,
                           None if pairs is None else functools.partial(self._pairs.expand, slot=ring))

    def _select_split(self, chunks, dev_in, labels, lo, hi, ring, pairs, tagged, rows):
        """--split_groups: {(mate, SPLIT): [grouped Piece]} - ONE grouped call per mate (two when a mate's files are part .gz, part
        plain) instead of a call per (mate, label)"""
        pieces, G, lab8 = {}, len(self._split_ids), labels.view(torch.int8)
        for e, plan in self._split_plan.items():
            text, table, _ = self._output_view(chunks, dev_in, None, e, lo, hi, ring, pairs, tagged)
            stride = 1 if pairs is None else 2                      # unit u's row is mate 1's: record u, or record 2 u of an interleaved chunk
            mate = e if pairs is not None and len(self.output) == 2 else -1
            for gz, slots, labs in plan:
                keys, kinfo = self._split.keys(rows, lab8, slots, G, 0, stride, mate, slot=(e, gz, ring))
                call = self._split.compress_grouped if gz else self._split.pack_grouped
                out, tab, info = call(text, table, keys, len(labs) * (G + 1), slot=(e, gz, ring))
                pieces.setdefault((e, SPLIT), []).append(Piece(out, _pinned(info), not gz, key_tab=_pinned(tab), kinfo=_pinned(kinfo), labels=labs))
        return pieces

    def _split_counted(self, e, labs, records):
        """the records per key of one grouped call, added to the run's counters (mate e's writer thread)"""
        G1 = len(self._split_ids) + 1
        for s, lab in enumerate(labs):
            self._split_recs[(e, lab)] += records[s * G1:(s + 1) * G1]

    def _select_chunk(self, chunks, dev_in, labels, lo, hi, on_dev, ring, pairs=None, tagged=None, rows1=None):
        """{(mate, label): [Piece]}: the label files whose records of this chunk are selected on the device, on the post stream beside
        the next chunk's recurrences, so that only the selected bytes travel to the host. A chunk whose text lives on the device: every
        file's, deflated (.gz outputs: BGZF members, csrc/rd_deflate.hpp) or packed into one text (rd_select_pack). Otherwise the .gz
        outputs' only - under the label gather: of this rank's shard (reference: gzip.open(..., compresslevel=5) on the host,
        detect.py:729-741). Every rank takes the same decision (the chunks of a shared decode are the same chunks)."""
        if self._split is not None:
            if not on_dev:
                raise RuntimeError("--split_groups: the chunk's text is not on the device (BAM input is device ingest only)")
            return self._select_split(chunks, dev_in, labels, lo, hi, ring, pairs, tagged, rows1)
        if on_dev:
            files = self._out_files
        elif self._gz_files and all(c.tensors is not None and len(c.tensors) > 3 and c.verbatim for c in chunks):
            files = self._gz_files
        else:
            return {}
        # (own writer: half of the worst-case output size is reserved - an incompressible chunk falls back to the host's deflate; under
        # the label gather the full bound, every rank must take the same path; a chunk on the device has no host text to fall back to)
        frac = 1.0 if on_dev or self.gathers_labels else 0.5
        pieces = {}
        views = {}                                  # mate -> (text, record table, labels) that select the records of its files
        for e, lab in files:
            if e not in views:                      # once per chunk and mate
                views[e] = self._output_view(chunks, dev_in, labels.view(torch.int8), e, lo, hi, ring, pairs, tagged)
            text, rs, sel = views[e]
            gz = (e, lab) in self._gz_files
            if gz:
                out, info = self._gz.compress_selected(text, rs, sel, lab, slot=(e, lab, ring), out_frac=frac)
            else:
                out, info = self._sel.pack_selected(text, rs, sel, lab, slot=(e, lab, ring))
            info = _pinned(info)
            pieces[(e, lab)] = [Piece(out, info, not gz, info, "gzip" if gz else "select")]
        return pieces

    def _report_chunk(self, chunks, dev_in, outs, labels, lo, hi, ring, pairs=None):
        """--read_report: the pieces of the lines of records [lo, hi) of the chunk, formatted where mate 1's text, its record starts
        and the final logits already are (rd_report_format, on the post stream after the float64 pass and the pair fusion), then
        deflated there too for a .gz report (its line starts are a record table of the report text: rd_gz_compress_selected of all of
        it; members that do not fit the reserved half fall back to the text, which the host deflates). Own buffers in the chunk's ring
        slot: the label files' are not shared."""
        source, pair_table = self._fastq_view(chunks, dev_in, 0, lo, hi, pairs)
        # (a line per unit: mate 1's records, or the pairs of an interleaved chunk as its records - whatever the outputs are)
        text, rs, _ = record_view(source, hi - lo, labels, 0, pairs is not None, 1, pair_table)
        rep, line_start, info = self._report.format(text, rs, outs[0][0], outs[1][0] if self.is_paired else None, labels.view(torch.int8), slot=ring)
        fault = _pinned(info)
        piece = Piece(rep, fault, True, fault, "report")
        if self._rep_gz:
            out, ginfo = self._gz.compress_selected(rep, line_start, self._report.zeros(hi - lo), 0, slot=REPORT + (ring,),
                                                    out_frac=1.0 if self.gathers_labels else 0.5)
            piece = Piece(out, _pinned(ginfo), False, fault, "report", fallback=piece)
        return [piece]

    def _regions_chunk(self, chunks, dev_in, plans, lo, hi, pairs=None, ring=None, need=None):
        """--regions: the piece of the region lines of units [lo, hi) of the chunk, formatted where the records' text, the reads'
        lengths, the window plans and the windows' final logits already are (rd_region_format, on the post stream after the float64
        pass), and the RegionRepeat that _finish_regions reads. Own buffer in the chunk's ring slot. The lines have no bound in the
        text's bytes, so a hint sizes the buffer (RD_REGIONS_HINT, else regions.default_hint) and _finish_regions formats the chunk
        again - need = the bytes the first call asked for, no ring slot: a buffer of its own - when it was too small. A .gz file: the
        text goes to the host's writer, which deflates it."""
        # The sources are record_view's, its answer is not: rd_region_format selects nothing by label, it walks every record of a mate. An
        # interleaved chunk's mate has the full table from entry e on, read with a stride of 2 - record_view skips the other mate by label.
        tabs = [self._fastq_view(chunks, dev_in, e, lo, hi, pairs)[0] for e in range(len(dev_in))]
        stride = 1 if pairs is None else 2
        if pairs is not None:
            tabs[1] = (tabs[1][0], tabs[1][1][1:])
        args = []
        for (text, rs), (_, _, ln), plan in zip(tabs, dev_in, plans):
            args += [text, rs, ln, plan]
        if need is None:
            text_bytes = sum(int(t.numel()) for t, _ in tabs[:1 if stride == 2 else 2])
            cap = _regmod.default_hint(text_bytes, hi - lo, sum(p["total"] for p in plans), len(plans))
        else:
            cap = int(need)
        buf = self._reg_out.get(ring)
        if buf is None or buf.numel() < cap:
            buf = torch.empty(((cap * 5 // 4 + 255) // 256) * 256, dtype=torch.uint8, device=self.device)
            if ring is not None:
                self._reg_out[ring] = buf
        # (a hint from the environment is taken at its word, also where the ring's buffer has grown beyond it)
        out, info = self.model.window_regions(*args, rec_stride=stride, out=buf, out_cap=cap if os.environ.get(_regmod.HINT_ENV) and need is None else None)
        info = _pinned(info)
        return Piece(out, info, True, info, "regions"), RegionRepeat(info, chunks, dev_in, plans, lo, hi, pairs)

    def _finish_regions(self, pieces, reg):
        """the verdict of rd_region_format on this rank's units of a chunk (the ticket's "regions" check), once the event behind it has
        passed: the counters are added up; lines that did not fit (fault 1) are formatted once more with the bytes they need, and
        their piece replaces the first one among the ticket's pieces before they are handed to the writer or the gather"""
        info = reg.info
        if int(info[3]) == 1:
            self.regions_repeats += 1
            post = self._post_stream
            with torch.cuda.stream(post):
                piece, reg = self._regions_chunk(reg.chunks, reg.dev_in, reg.plans, reg.lo, reg.hi, reg.pairs, need=int(info[1]))
                done = _native_mod.new_event()
                done.record(post)
            _native_mod.wait_event(done)
            info, pieces[REGIONS] = reg.info, [piece]
        if int(info[3]):
            raise RuntimeError("device regions: the chunk's record tables, lengths or window plans do not describe its text (fault %d)" % int(info[3]))
        for k in range(4):
            self._reg_counts[k] += int(info[4 + k])

    def collect_chunk(self, tk):
        """Labels of a submitted chunk: int8 numpy on rank 0 (whole chunk, input order), None elsewhere. The host waits for the chunk's
        `done` event (the label gather of a chunk without checks: in the collectives alone), then every rank runs its shard's checks."""
        if tk.checks or not self.gathers_labels:
            _native_mod.wait_event(tk.done)        # (a blocking event: the thread sleeps in the driver, it does not spin a host core)
        tk.run_checks()
        if not self.gathers_labels:
            return tk.host.numpy()
        labels = tk.finish()
        if tk.pieces:
            self._gather_pieces(tk)
        return None if self.rank != 0 else labels.cpu().numpy()

    @staticmethod
    def _check_totals(totals):
        """the verdict of rd_fastq_gather on a device chunk's views (pinned totals; None: no such view), once its `ready` event has passed"""
        if any(t is not None and int(t[0]) < 0 for t in totals):
            raise RuntimeError("device chunk assembly failed (rd_fastq_gather)")

    @staticmethod
    def _check_counted(what, info):
        """the verdict of rd_summary_accumulate / rd_bam_group_accumulate on this rank's units of a chunk, once the event behind it passed"""
        if int(info[0]):
            raise RuntimeError("device %s are not what the counters can take (fault %d); nothing of the chunk was counted" % (what, int(info[0])))

    def _gather_pieces(self, tk):
        """label gather: the pieces every rank made of its shard travel to rank 0, which appends them in rank order = input order
        (sizes first: one small all-gather per chunk; then one padded gather per output file)"""
        _native_mod.wait_event(tk.done)
        pieces = tk.pieces
        own = [(key, pieces[key][0]) for key in pieces]
        mine = [p.size() for _, p in own]
        sizes = rdist.all_gather_sizes(mine)
        for f, (key, p) in enumerate(own):
            if mine[f] > p.buf.numel():
                raise RuntimeError("device gzip: output buffer too small (%d > %d)" % (mine[f], p.buf.numel()))
            parts = rdist.gather_var_bytes(p.buf, mine[f], sizes[:, f].tolist(), dst=0)
            pieces[key] = [p._replace(buf=t, info=None, fault=None, fallback=None) for t in parts or ()]

    def classify_chunk(self, chunks):
        """chunks: (c1,) or (c1, c2). Returns the int8 labels of the whole chunk on rank 0 (numpy), None elsewhere."""
        return self.collect_chunk(self.submit_chunk(chunks))

    # ---- drivers ----------------------------------------------------------------------------------------
    # Host pipeline: one parser thread per input file -> GPU (main thread) -> one writer thread per mate. The C++ reader,
    # the kernels and the C++ writer all release the GIL, so the three stages overlap (the reference parses the two mates
    # with Pool(2), detect.py:131-132, but encodes, classifies and writes in lock-step).
    @staticmethod
    def _spawn(target, *a):
        th = threading.Thread(target=target, args=a, daemon=True)
        th.start()
        return th

    def _reader_queue(self, path, chunk_reads, depth=2, byte_range=None, arena=None, schedule=None):
        q = queue.Queue(maxsize=depth)
        # --interleaved: every chunk size doubled (the first chunk and the growth steps too), so that a chunk holds an even number of
        # records and chunk_reads PAIRS - the chunk boundaries of the two-file run, in pairs
        mul = 2 if self.interleaved else 1
        chunk_reads, first = chunk_reads * mul, (1 << 17) * mul

        def work():
            try:
                self._mark("reader_thread_%s" % os.path.basename(str(path)))
                # FASTQ whose text can stay on the device (plain files, BGZF): H2D of the file's bytes, members inflated and records
                # framed there - no parser thread at all (data_loader/device_reader.py; RD_DEVICE_PARSE=0 keeps the host parser)
                if arena is None and self._device_parse(path):
                    st = self.ingest.setdefault(os.path.basename(str(path)), {"path": "device"})
                    stream = dr.get_seq_chunks_device(path, chunk_size=chunk_reads, byte_range=byte_range, first_chunk=first, schedule=schedule,
                                                      device=self.device, stats=st, keep_raw=self.bam_output or self.read_groups or self.split_groups or self.bam_tags is not None,
                                                      rank=self.rank if self.sharded_parse else None)
                # one plain input file: its parser thread was the slowest stage of the pipeline - two readers over byte segments,
                # small first chunks (mate files keep one reader each and exact chunk sizes: their chunks must pair up)
                # (not an interleaved file: its chunks must hold whole pairs)
                elif arena is None and len(self.input) == 1 and not self.interleaved and not fx.file_info(path)[1] and int(self.args.threads) >= 4:
                    stream = fx.get_seq_chunks_parallel(path, chunk_size=chunk_reads, byte_range=byte_range, workers=2)
                else:
                    stream = fx.get_seq_chunks(path, chunk_size=chunk_reads, byte_range=byte_range, first_chunk=first, arena=arena,
                                               schedule=schedule, device=self.device)
                for c in stream:
                    q.put(c)
                q.put(None)
            except BaseException as e:      # surface parser errors on the main thread
                q.put(e)
            finally:
                self.thread_cpu_s["reader:" + os.path.basename(str(path))] = round(time.thread_time(), 4)
        self._spawn(work)
        return q

    def _device_parse(self, path):
        """does this input's text stay on the device? FASTQ, plain or BGZF, when every record a rank reads is a record it classifies
        (one rank, or the sharded parse) - under the label gather the chunk's lengths are needed on the host for the shard bounds"""
        if self._use_device is None:      # ONE decision for the run: the mates' chunks must be of one kind (submit_chunk looks at the first)
            self._use_device = not self.gathers_labels and all(dr.device_parse_wanted(p) for p in self.input)
        return self._use_device

    def _shared_decode(self):
        """several ranks of ONE node on gzip input: rank 0 inflates and parses the stream once into shared memory (fx.ShmArena)
        and tells the others where each chunk lies; they map it and take their share of the records. (Ranks spread over several
        nodes cannot share memory: there every rank decodes the stream itself, as in round 2.)"""
        if self._shared is None:
            # one node only - and only when the launcher SAYS so (torchrun sets LOCAL_WORLD_SIZE; a launcher that sets just
            # RANK / WORLD_SIZE may have spread the ranks over several hosts, whose /dev/shm are different memories)
            ok = (self.gathers_labels and self.world > 1 and os.environ.get("RD_SHARED_DECODE", "1") != "0" and
                  os.environ.get("LOCAL_WORLD_SIZE") is not None and int(os.environ["LOCAL_WORLD_SIZE"]) == self.world)
            if ok:                                   # rank 0 owns the slots: its /dev/shm must hold them (all ranks take its answer)
                msg = [None]
                if self.rank == 0:
                    fx.ShmArena.sweep_stale()
                    chunk = (self._chunk_reads or DEFAULT_CHUNK_READS) * (2 if self.interleaved else 1)
                    fits, need = fx.ShmArena.fits(len(self.input), chunk, 2 * max(self.len, 50) + 80)
                    msg = [bool(fits)]
                    if not fits:
                        self.logger.info('Shared gzip decode needs about {} MB of /dev/shm, which is not free: every rank decodes '
                                         'the input itself'.format(need >> 20))
                dist.broadcast_object_list(msg, src=0)
                ok = bool(msg[0])
            self._shared = ok
        return self._shared

    def _chunk_stream(self, chunk_reads):
        shared = self._shared_decode()
        if shared and self.rank != 0:                # chunks arrive as descriptions of rank 0's shared-memory slots
            while True:
                msg = [None]
                t0 = time.perf_counter()
                dist.broadcast_object_list(msg, src=0)
                self._stage_s["wait_reader"] += time.perf_counter() - t0
                if msg[0] is None:
                    return
                if isinstance(msg[0], str):
                    raise RuntimeError("rank 0: " + msg[0])
                yield tuple(fx.ShmArena.attach(d) for d in msg[0])
        ranges = self._ranges if self.sharded_parse else [None] * len(self.input)
        # -t/--threads also bounds the decoder threads of .gz inputs (parallel DEFLATE decoding, csrc/rd_pgzip.h): what is left after
        # the parser threads and this one, divided among the input files - and among the ranks when every rank decodes for itself
        sharers = len(self.input) * (1 if shared else self.world)
        _native_mod.host_lib().rd_host_set_gz_threads(max(2, min(12, (int(self.args.threads) - 2) // max(1, sharers))))
        arenas = [None] * len(self.input)
        if shared:
            tag = "rd_%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.getpid())
            arenas = [fx.ShmArena("%s_f%d" % (tag, i)) for i in range(len(self.input))]
            self._arenas += arenas
        schedule = None
        if len(self.input) == 2 and not shared and not any(fx.file_info(p)[1] for p in self.input):
            # plain mate files: one schedule of chunk sizes for both readers (small first AND last chunks), from the first file
            schedule = fx.chunk_schedule(self.input[0], chunk_reads, byte_range=ranges[0]) or None
        qs = [self._reader_queue(p, chunk_reads, byte_range=r, arena=a, schedule=schedule) for p, r, a in zip(self.input, ranges, arenas)]
        while True:
            cs = []
            err = None
            for q in qs:
                t0 = time.perf_counter()
                c = q.get()
                self._stage_s["wait_reader"] += time.perf_counter() - t0
                if isinstance(c, BaseException):
                    err = c
                    break
                cs.append(c)
            if err is None and not all(c is None for c in cs) and (any(c is None for c in cs) or len({len(c.seq_len) for c in cs}) != 1):
                err = ValueError("paired-end files have different numbers of records")
            if shared:                                # (an error is passed on, so that no rank waits for a chunk that never comes)
                dist.broadcast_object_list([str(err) if err is not None else None if cs[0] is None else [c.shm for c in cs]], src=0)
            if err is not None:
                raise err
            if all(c is None for c in cs):
                return
            yield tuple(cs)

    def _interleaved_chunks(self, stream):
        """--interleaved: the chunks of the one file, each with an even number of records. Only the file's last chunk can be odd: its
        pairs are classified and written like any other's, and the run ends with the error (check_even_records) afterwards."""
        seen = 0
        for (c,) in stream:
            if seen % 2:
                raise RuntimeError("interleaved input: a chunk with an odd number of records was not the last one")
            self._chunk_first_record, seen = seen, seen + len(c.seq_len)
            self._records_seen = seen
            if fx.interleaved_pairs(c):
                yield (c,)
            elif c.release is not None:              # (a lone last record)
                c.release()

    def _writer_items(self, chunks, labels):
        """what every writer thread gets of a chunk: (chunk, labels) whose records of one label are its files' - what the host writes
        itself (fh.write_selected: plain outputs of host-parsed chunks, device pieces that did not fit). The layouts are record_view's,
        over chunks instead of tables: fx.pair_view and fx.expand_pair_labels are the host's forms of its two interleaved answers."""
        if not self.interleaved:
            return [(chunks[e], labels) for e in range(len(self.output))]
        c = chunks[0]
        if isinstance(c, dr.DeviceChunk):            # (everything comes from the device; there is no host text)
            return [(c, labels)] * len(self.output)
        if len(self.output) == 1:                    # interleaved output: the pairs are the records
            return [(fx.pair_view(c), labels)]
        # split output: both writers hold the full chunk, each with its mate's expanded labels; the chunk is released by the second
        left, lock = [2], threading.Lock()

        def release():
            with lock:
                left[0] -= 1
                last = left[0] == 0
            if last:
                c.release()
        both = c if c.release is None else c._replace(release=release)
        return [(both, fx.expand_pair_labels(labels, e)) for e in (0, 1)]

    def run_with_chunks(self, chunk_reads=None):
        """Classify the input in chunks and write the outputs (reference detect.py:326-523)."""
        if chunk_reads is None:
            chunk_reads = self.batch_size * self.chunk_size
        self._chunk_reads, self._shared, self._use_device = chunk_reads, None, None
        self._timeline, self._t_run = [], time.perf_counter()
        self._plan_ranks()
        _native_mod.host_lib().rd_host_set_threads(int(self.args.threads))   # -t/--threads: gzip workers; read when a writer is opened
        writes = self.rank == 0 or not self.gathers_labels
        files = self._open_outputs() if writes else []     # [((mate, label), final path, handle)]
        counts = [0, 0, 0, 0]                      # num_read, num_nonrrna, num_rrna, num_unknown
        self._mark("outputs_open")
        self._stage_s = {"wait_reader": 0.0, "classify": 0.0, "wait_writer": 0.0}   # main-thread seconds per pipeline stage
        self.thread_cpu_s = {}                                                      # CPU seconds of the pipeline's Python threads, by role
        main_cpu0 = time.thread_time()
        self._first_chunk = None
        self.ingest = {}                           # per input file: which reader took it, and the device feeder's stage times
        self._copy_stream = _gzmod.acquire_stream(self.device)      # (pooled: the allocator's cache is per stream, gz.acquire_stream)
        self._post_stream = _gzmod.acquire_stream(self.device)
        self._device_outputs([key for key, _, _ in files if key not in TEXT_FILES])
        # writer threads (rank 0; every rank under the sharded parse): one per mate, records of every label file in input order
        errors = []
        writers = [_MateWriter(self, e, [(key, fh) for key, _, fh in files if key[0] == e], errors)
                   for e in range(len(self.output))] if writes else []      # (one per mate file; an interleaved output is one file)
        self._mark("writers_started")
        stream = self._chunk_stream(chunk_reads)
        self._records_seen, mismatch = 0, None
        try:
            for chunks, tk in self._in_flight(self._interleaved_chunks(stream) if self.interleaved else stream):
                t0 = time.perf_counter()
                try:
                    labels = self.collect_chunk(tk)
                except (MateMismatch, UbamRecordError) as e:      # the chunks in front of this one are written and the files closed, then the error
                    mismatch = e
                    break
                self._mark("labels")
                self._stage_s["classify"] += time.perf_counter() - t0
                counts[0] += tk.n
                if self._first_chunk is None:
                    self._first_chunk = (time.perf_counter(), counts[0])
                if writes:
                    if errors:
                        raise errors[0]
                    for i, lab in enumerate((0, 1, -1), 1):
                        counts[i] += int((labels == lab).sum())
                    t0 = time.perf_counter()
                    for w, (c, lab) in zip(writers, self._writer_items(chunks, labels)):
                        w.q.put((c, lab, tk.pieces))
                    self._stage_s["wait_writer"] += time.perf_counter() - t0
                    if self.rank == 0:
                        self.logger.info('{}{}{} sequences finished!'.format(colors.OKGREEN, counts[0], colors.ENDC))
        finally:
            for w in writers:
                w.q.put(None)
            for w in writers:
                w.thread.join()
            # (given back in the order they were taken: the pool is last-in first-out, so the streams come back in the same roles every
            # other run - and with them the allocator's blocks cached per stream)
            for st in [self._copy_stream, self._post_stream] + [w.stream for w in writers]:
                try:
                    st.synchronize()
                except Exception:      # noqa: BLE001 - (a failed run: the stream is given back all the same)
                    pass
                _gzmod.release_stream(st)
        if errors:
            raise errors[0]
        if mismatch is not None:
            for _, _, fh in files:
                fh.close()
            raise mismatch
        self.thread_cpu_s["main"] = round(time.thread_time() - main_cpu0, 4)
        self._close_arenas()
        if writes:
            self.writer_threads = sorted({fh.threads for key, _, fh in files if key not in TEXT_FILES})
            for _, _, fh in files:
                fh.close()
        if self.sharded_parse:
            counts = self._join_parts(counts, [path for _, path, _ in files])
        self.num_read, self.num_nonrrna, self.num_rrna, self.num_unknown = counts
        if self.rank == 0:
            self.logger.info('Processed {}{}{}{} sequences in total'.format(colors.BOLD, colors.OKCYAN, self.num_read, colors.ENDC))
            self.logger.info('Detected {}{}{}{} non-rRNA sequences'.format(colors.BOLD, colors.OKCYAN, self.num_nonrrna, colors.ENDC))
            self.logger.info('Detected {}{}{}{} rRNA sequences'.format(colors.BOLD, colors.OKCYAN, self.num_rrna, colors.ENDC))
            if self.is_paired and self.args.ensure == 'both':
                self.logger.info('Discarded {}{}{}{} unclassified sequences'.format(
                    colors.BOLD, colors.OKCYAN, self.num_unknown, colors.ENDC))
        # The counters of every rank's own share, summed over the ranks (_sum_ranks). Which flag says that the shares differ: BAM records
        # and tags are counted where the file is framed, and BAM input under several ranks is the sharded parse only (--bam_shard;
        # check_bam) - sharded_parse. Windows and regions are counted where units are classified: both layouts of several ranks - multi.
        bam_in = [path for path in self.input if fx.get_seq_format(path) == "bam"]
        if bam_in:                                 # (one rank, or --bam_shard: every rank walked the records of its share)
            total = self._sum_ranks([((self.ingest.get(os.path.basename(str(path))) or {}).get("indexer") or {}).get(k, 0)
                                     for path in bam_in for k in ("bam_records", "bam_skipped")], self.sharded_parse)
            for f, path in enumerate(bam_in):
                if self.rank == 0:
                    self.logger.info('BAM input: {} records, {} secondary/supplementary skipped ({})'.format(total[2 * f], total[2 * f + 1], path))
        if self._tags is not None:                 # --bam_tags: every rank tagged the records of its own share
            total = self._sum_ranks(_tagmod.as_vector([t.counts() for t in self._tags], len(self.bam_tags)).tolist(), self.sharded_parse)
            self._tag_total = _tagmod.from_vector(total, len(self.bam_tags), len(self._tags))
            if self.rank == 0:
                self.logger.info(_tagmod.log_line(self.bam_tags, self._tag_total))
        if self._ubam is not None:                 # --ubam_output: one rank
            self._ubam_total = [u.counts for u in self._ubam]
            self.logger.info(_ubammod.log_line(self._ubam_total))
            if self.ubam_tags:
                self._ubam_tag_total = [u.tag_counts() for u in self._ubam]
                self.logger.info(_ubammod.log_line_tags(self.ubam_tags, self._ubam_tag_total))
        if self.interleaved:
            fx.check_even_records(self._records_seen)
        if self._split is not None:
            self._split_total = self._finish_split(sum(1 for key, _, _ in files if len(key) == 3))
        mates = range(2 if self.is_paired else 1)
        if self._windows is not None:              # every rank classified the windows of its own shard / byte range
            total = self._sum_ranks(self._win_classified, self.multi)
            self._win_total = [total[e] for e in mates]
            if self.rank == 0:
                self.logger.info('Classified {}{}{}{} windows ({} mode, at most {} per read)'.format(
                    colors.BOLD, colors.OKCYAN, " + ".join(str(x) for x in self._win_total), colors.ENDC, self._windows["fuse"],
                    self._windows["max_per_read"]))
        if self._regions:                          # likewise: every rank formatted the regions of its own units
            total = self._sum_ranks(self._reg_counts, self.multi)
            self._reg_total = [[total[k + e] for e in mates] for k in (0, 2)]
            if self.rank == 0:
                self.logger.info('Wrote {}{}{}{} rRNA regions in {} reads'.format(
                    colors.BOLD, colors.OKCYAN, " + ".join(str(x) for x in self._reg_total[0]), colors.ENDC,
                    " + ".join(str(x) for x in self._reg_total[1])))
        if self._summary is not None:
            self._write_summary()

    def _finish_split(self, n_files):
        """--split_groups, at the end of a run that went well: the records every family received, summed over the chunks, against the
        run's own counts per class - a file of a mate gets one record per unit of its class -; the log line; the summary's object"""
        want = {0: self.num_nonrrna, 1: self.num_rrna, -1: self.num_unknown}
        for (e, lab), recs in sorted(self._split_recs.items()):
            if int(recs.sum()) != want[lab]:
                raise RuntimeError("--split_groups: the files of mate {} for label {} received {} records, the run counted {} units".format(
                    e + 1, lab, int(recs.sum()), want[lab]))
        G = len(self._split_ids)
        # units by class in the unassigned member (mate 1's files; None: the run writes no file for the class)
        un = {name: (int(self._split_recs[(0, lab)][G]) if (0, lab) in self._split_recs else None)
              for name, lab in (("unclassified", -1), ("nonrRNA", 0), ("rRNA", 1))}
        self.logger.info('Split outputs: {} read groups + unassigned, {} files; {} reads unassigned'.format(
            G, n_files, sum(v for v in un.values() if v is not None)))
        return {"groups": G, "files": n_files, "unassigned": un}

    def _write_summary(self):
        """--summary, at the end of a run that went well (every output file is closed): the ranks' counters summed, checked against
        the run's own counts and written by rank 0 as JSON"""
        acc = self._summary.acc
        gacc = None if self._groups is None else self._groups.acc      # (BAM input: one rank, or --bam_shard - the groups of a rank's share)
        if self.multi:                             # every rank counted its own shard / byte range
            acc = rdist.reduce_counts(acc)
            gacc = None if gacc is None else rdist.reduce_counts(gacc)
        if self.rank != 0:
            return
        gacc = None if gacc is None else gacc.cpu().numpy()
        acc = acc.cpu().numpy()
        units = [int(x) for x in _summod.sections(acc)["units"]]
        if units != [self.num_unknown, self.num_nonrrna, self.num_rrna]:
            raise RuntimeError("--summary: the device counted {} unclassified / non-rRNA / rRNA units, the run {}".format(
                units, [self.num_unknown, self.num_nonrrna, self.num_rrna]))
        path = self.summary_path
        doc = _summod.to_json(acc, {"version": __version__, "paired": bool(self.is_paired), "interleaved": self.interleaved, "len": int(self.len),
                                    "ensure": self.args.ensure, "model": self.state_key, "inputs": list(self.input),
                                    "windows": None if self._windows is None else dict(
                                        self._windows, stride=int(self._windows["stride"] or self.len), classified=list(self._win_total),
                                        **({"regions": list(self._reg_total[0]), "reads_with_regions": list(self._reg_total[1])}
                                           if self._regions else {}))})
        if self._groups is not None:
            grp = self._groups
            got = _grpmod.units_per_class(gacc, grp.G)
            if got != units:
                raise RuntimeError("--read_groups: the rows of the read groups hold {} unclassified / non-rRNA / rRNA units, the run {}".format(got, units))
            rg = doc["read_groups"] = _grpmod.to_json(gacc, grp.groups, bool(self.is_paired), input=self.input[0])
        if self._tags is not None:
            doc["bam_tags"] = _tagmod.to_json(self.bam_tags, self._tag_total, floats=self.bam_tag_floats)
        if self._split is not None:
            doc["split_groups"] = self._split_total
        if self._ubam is not None:
            doc["ubam_output"] = _ubammod.to_json(self._ubam_total)
            if self.ubam_tags:
                doc["ubam_tags"] = _ubammod.to_json_tags(self.ubam_tags, self._ubam_tag_total, floats=self.ubam_tag_floats)
        _summod.write_json(path, doc)
        frac = doc["reads"]["rRNA_fraction"]
        self.logger.info('rRNA fraction: {} (summary: {})'.format("n/a" if frac is None else "%.6f" % frac, path))
        if self._groups is not None:
            self.logger.info('Read groups: {} declared, {} with reads; {} reads without RG, {} undeclared, {} with malformed tags'.format(
                len(rg["groups"]), sum(1 for g in rg["groups"] if g["units"]["total"]), rg["none"]["units"]["total"],
                rg["undeclared"]["units"]["total"], rg["malformed_tags"]["units"]["total"]))

    def _mark(self, event, t=None):
        """the first events of the run on its timeline, seconds since it started (timing first_chunks_timeline: tools/first_chunk_probe.py)"""
        if len(self._timeline) < 30:
            self._timeline.append((event, round((time.perf_counter() if t is None else t) - self._t_run, 4)))

    def _all_gather(self, obj):
        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out

    def _sum_ranks(self, mine, shares):
        """a list of integers, one list per rank -> their sums per column; shares: do the ranks hold different shares (a collective
        that every rank calls) - else this rank's list is the whole run's"""
        per_rank = self._all_gather(mine) if shares else [mine]
        return [sum(int(r[k]) for r in per_rank) for k in range(len(mine))]

    def _plan_ranks(self):
        """How the ranks share the input - the run's layout (module docstring): sets sharded_parse and, under it, this rank's share of
        every input file (_ranges, bytes_parsed). Every rank calls it (collectives)."""
        if self.interleaved and self.multi:
            # byte ranges of an interleaved file would have to be cut at even record counts: one decode (per node, or per rank), host
            # chunks, and every rank classifies a shard of each chunk's PAIRS
            self.sharded_parse, self.bytes_parsed = False, None
            if self.rank == 0:
                self.logger.info('--interleaved input: the ranks take the label-gather layout (one decode, every rank classifies a shard '
                                 'of the pairs of each chunk)')
            return
        # plain inputs under several ranks: every rank parses, classifies and writes its own byte range (no label exchange)
        plain = not any(fx.file_info(p)[1] for p in self.input)
        # ... and BGZF FASTQ inputs likewise: their members are independent, so every rank inflates (on its own GPU), parses, classifies
        # and writes the members of its share (positions in the decompressed stream, fx.BgzfView). RD_BGZF_SHARD=0: one decoding rank
        bgzf = (self.multi and not plain and os.environ.get("RD_BGZF_SHARD", "1") != "0"
                and all(fx.get_seq_format(p) in ("fqgz", "fagz") and fx.bgzf_all_the_way(p) and fx.device_inflate_wanted(p) for p in self.input))
        # ... and BAM inputs under --bam_shard (check_bam: every input is BAM, RD_BGZF_SHARD is not 0): the same layout, with views that
        # find the record starts of a length-prefixed chain by a search on the GPU (data_loader/bam_shard.py)
        bam_in = self.multi and self.bam_shard and all(fx.get_seq_format(p) == "bam" for p in self.input)
        bgzf = bgzf or bam_in
        views = None
        if bgzf:                    # the member index: rank 0 walks the headers, the others receive the three arrays per file
            idx = [None]
            if self.rank == 0:
                try:
                    idx = [[fx.BgzfView.build_index(p) for p in self.input]]
                except ValueError as e:     # not BGZF all the way (a plain member in the middle): the one-decoder path reads such files
                    idx = [str(e)]
            dist.broadcast_object_list(idx, src=0)
            if isinstance(idx[0], str):
                if bam_in:                  # (no one-decoder path for BAM under several ranks: raised by every rank, from the same index)
                    raise RuntimeError("--bam_shard: {}: the file is not BGZF all the way - run on one rank".format(idx[0]))
                if self.rank == 0:
                    self.logger.info('{}: one rank decodes'.format(idx[0]))
                bgzf = False
            elif bam_in:
                from .data_loader import bam_shard
                views = [bam_shard.BamView(p, index=i, device=self.device) for p, i in zip(self.input, idx[0])]
            else:
                views = [fx.BgzfView(p, index=i) for p, i in zip(self.input, idx[0])]
        # ... and single-stream .gz inputs (what sequencers write; round 6): every rank decodes its own compressed range on its own GPU -
        # symbols first, bytes once the ranks have exchanged the 64 KiB maps of their ranges (data_loader/gz_shard.py). What the device
        # decoder does not take (or RD_GZ_SHARD=0) stays with the one-decode path (the label gather).
        gzr = None
        if (self.multi and not plain and not bgzf and os.environ.get("RD_GZ_SHARD", "1") != "0"
                and all(dr.device_ingest_kind(p) == "stream" for p in self.input)):
            from .data_loader import gz_shard
            t0 = time.perf_counter()
            gzr, why = gz_shard.prepare(self.input, self.rank, self.world, self.device, [fx.get_seq_format(p).startswith("fa") for p in self.input],
                                        self._all_gather, rdist.shift_to_prev)
            if gzr is None and self.rank == 0:
                self.logger.info('{}: one rank decodes'.format(why))
            self.gz_shard_s = time.perf_counter() - t0
            if gzr is not None:                      # (every rank says so itself: the line is what shows that no rank read another's bytes)
                self.logger.info('Rank {} decoded {} compressed bytes into {} bytes of text on {} in {:.2f} s'.format(
                    self.rank, ", ".join(str(x.comp_bytes) for x in gzr), ", ".join(str(x.stats["text_bytes"]) for x in gzr), self.device, self.gz_shard_s))
        self.sharded_parse = self.multi and (plain or bgzf or gzr is not None)
        self.bytes_parsed = None
        if self.sharded_parse:
            if gzr is not None:
                self._ranges = gzr
            else:
                self._ranges = fx.plan_ranges(self.input, self.rank, self.world, self._all_gather, views=views)
            self.bytes_parsed = [e - b for b, e in self._ranges]
            totals = [v.size for v in views] if views else [fx.file_info(p)[0] for p in self.input]
            for r, bp in enumerate(self._all_gather(self.bytes_parsed)):
                if self.rank == 0:
                    self.logger.info('Rank {} parses {} bytes of {}{}'.format(
                        r, ", ".join(str(b) for b in bp), ", ".join(str(t) for t in totals),
                        " (decompressed; BGZF members)" if bgzf else " (compressed; ranges of one DEFLATE stream)" if gzr is not None else ""))

    def _open_outputs(self):
        """Open this rank's output set - under the sharded parse its part of every file: the label files, the '.unclassified.gz'
        files (-e both, pairs) and the --read_report with its header. Returns [((mate, label), final path, handle)] in opening order."""
        files, headers = [], {}
        log = self.logger.info if self.rank == 0 else (lambda *a, **k: None)

        def open_(label, paths):               # one file per mate: keys (mate, label); the report's is REPORT
            split = self._split_ids is not None and label in (0, 1, -1)       # --split_groups: a family of files per label file
            members = [(e, g, m) for e, path in enumerate(paths) for g, m in enumerate(_bammod.split_paths(path, self._split_ids))] if split \
                else [(e, None, path) for e, path in enumerate(paths)]
            for e, g, path in members:
                if self.sharded_parse:
                    self._part_files.append(part_path(path, self.rank))
                files.append(((e, label) if g is None else (e, label, g), path,
                              fx.open_for_write(self._part_files[-1] if self.sharded_parse else path)))
                if self.sharded_parse:         # parts are joined later: the joined file gets ONE BGZF end-of-file block, at its end
                    files[-1][2].set_eof_marker(False)
                # a BAM output starts with the header of its mate's input, byte for byte (the sharded parse: rank 0's part comes first)
                if self.bam_output and label in (0, 1, -1) and (self.rank == 0 or not self.sharded_parse):
                    src = self.input[e if len(self.input) == 2 else 0]
                    if src not in headers:
                        headers[src] = np.frombuffer(_bammod.header(src), dtype=np.uint8)
                    files[-1][2].write_text(headers[src].ctypes.data, headers[src].size)
                elif self.ubam_output and label in (0, 1, -1):      # ... or with the one header of --ubam_output: no references, no @PG
                    hdr = np.frombuffer(_bammod.encode_header((), _bammod.UBAM_HEADER_TEXT), dtype=np.uint8)
                    files[-1][2].write_text(hdr.ctypes.data, hdr.size)
        if self.rrna is not None:
            log('Writing output rRNA sequences into file: {}{}{}'.format(colors.OKBLUE, ", ".join(self.rrna), colors.ENDC))
            open_(1, self.rrna)
        log('Writing output non-rRNA sequences into file: {}{}{}'.format(colors.OKBLUE, ", ".join(self.output), colors.ENDC))
        open_(0, self.output)
        if self.is_paired and self.args.ensure == 'both':
            unclf = [unclassified_path(path, self.bam_files) for path in self.output]
            open_(-1, unclf)
            log('Writing unclassified sequences into file: {}{}{}'.format(colors.OKYELLOW, ", ".join(unclf), colors.ENDC))
        rep_path, reg_path = self.report_path, self.regions_path
        if rep_path:
            log('Writing per-read report into file: {}{}{}'.format(colors.OKBLUE, rep_path, colors.ENDC))
            open_(REPORT[1], [rep_path])
            if self.rank == 0:                 # (the sharded parse: rank 0's part comes first in the joined file)
                hdr = np.frombuffer(_gzmod.REPORT_HEADER_PE if self.is_paired else _gzmod.REPORT_HEADER_SE, dtype=np.uint8)
                files[-1][2].write_text(hdr.ctypes.data, hdr.size)
        if reg_path:
            log('Writing rRNA regions into file: {}{}{}'.format(colors.OKBLUE, reg_path, colors.ENDC))
            open_(REGIONS[1], [reg_path])
            if self.rank == 0:
                hdr = np.frombuffer(_regmod.HEADER, dtype=np.uint8)
                files[-1][2].write_text(hdr.ctypes.data, hdr.size)
        return files

    def _device_outputs(self, out_files):
        """what the GPU makes of the outputs: which (mate, label) files it deflates or packs, and the --read_report's lines"""
        # which (mate, label) files are gzip outputs deflated on the device: every rank deflates the records it classified - and writes
        # them itself (one rank, or the sharded parse) or, under the label gather, sends the members to rank 0
        self._gz_files = []
        self._chunk_seq = 0                        # chunks submitted (submit_chunk): chunk k's buffers are those of ring slot k % GZ_RING
        if self.gzip_on_device:                    # (the same list on every rank: it is derived from the arguments)
            self._gz_files = self.gz_output_files(self.output, self.rrna, self.is_paired, self.args.ensure)
        # every (mate, label) file this run writes; for chunks on the device the plain ones are packed there (rd_select_pack)
        self._out_files = out_files
        if any(self._device_parse(p) for p in self.input):
            self._sel = _gzmod.DeviceSelect(self.device)
        self._pairs = _gzmod.DevicePairSplit(self.device) if self.interleaved else None
        # --read_report: one line per read (pair), formatted on the device for every chunk; mate 1's writer appends the pieces
        rep_path = self.report_path
        self._report = _gzmod.DeviceReport(self.device) if rep_path else None
        self._rep_gz = bool(rep_path) and self.gzip_on_device and rep_path.endswith('gz')      # (else the host's writer deflates a .gz report)
        # --summary: the run's QC counters, one int64 array per rank that every chunk adds to on the post stream
        self._summary = _summod.DeviceSummary(self.device) if self.summary_path else None
        # --read_groups: the same units per read group of mate 1's BAM, one more int64 array that every chunk adds to
        self._groups = _grpmod.DeviceGroups(self.device, _bammod.header(self.input[0])) if self.read_groups else None
        # --split_groups: per mate the grouped calls of its family files - (gzip?, class_slot, labels in slot order) - and the counters
        if self._split_ids is not None:
            G, gzset = len(self._split_ids), set(self.gz_output_files(self.output, self.rrna, self.is_paired, self.args.ensure))
            if gzset and not self.gzip_on_device:
                raise RuntimeError("--split_groups: compressed family files are deflated on the device only (kernel.gzip / RD_DEVICE_GZIP = host)")
            self._split = _gzmod.DeviceGroupSelect(self.device)
            self._split_dict = self._groups.dict if self._groups is not None else _grpmod.Dictionary(self.device, self._split_ids)
            self._split_plan, self._split_recs = {}, {}
            for e in sorted({key[0] for key in out_files}):
                labs_e = [key[1] for key in out_files if key[0] == e and key[2] == 0]
                self._split_plan[e] = []
                for gz in (True, False):
                    labs = tuple(lab for lab in labs_e if ((e, lab) in gzset) == gz)
                    if labs:
                        slots = [-1, -1, -1]
                        for k, lab in enumerate(labs):
                            slots[lab + 1] = k
                        self._split_plan[e].append((gz, slots, labs))
                for lab in labs_e:
                    self._split_recs[(e, lab)] = np.zeros(G + 1, dtype=np.int64)
        # --bam_tags: the tagged view of every chunk, and the counters of the tags copied, per input file
        self._tags = [_tagmod.DeviceBamTags(self.device, self.bam_tags, floats=self.bam_tag_floats) for _ in self.input] if self.bam_tags is not None else None
        # --ubam_output: the raw view of every chunk is made of its text, and the counters of what the BAM form changed, per input file
        self._ubam, self._ubam_seen = None, 0
        if self.ubam_output:
            self._ubam = [_ubammod.DeviceUbam(self.device, fasta=fx.get_seq_format(p).startswith("fa"), tags=self.ubam_tags or (), floats=self.ubam_tag_floats) for p in self.input]
        self._win_classified = [0, 0]
        # --regions: the lines of every chunk, formatted on the device; mate 1's writer appends the pieces (and deflates a .gz file)
        self._regions = bool(self.regions_path)
        self._reg_out, self._reg_counts, self.regions_repeats = {}, [0, 0, 0, 0], 0
        if self._gz_files or self._rep_gz:
            self._gz = _gzmod.DeviceGzip(self.device)

    def _in_flight(self, stream):
        """chunk k+1 is submitted (its H2D starts) before the labels of chunk k are waited for"""
        prev = None
        for seq, chunks in enumerate(stream):
            t0 = time.perf_counter()
            self._mark("chunk_of_%d_read" % len(chunks[0].seq_len), t0)    # (the first chunks' way through the pipeline)
            tk = self.submit_chunk(chunks, seq)
            self._mark("submitted")
            self._stage_s["classify"] += time.perf_counter() - t0
            if prev is not None:
                yield prev
            prev = (chunks, tk)
        if prev is not None:
            yield prev

    def _join_parts(self, counts, finals):
        """sharded parse: the four counters summed over the ranks (returned), and every output file joined from the ranks' parts"""
        tot = torch.tensor(counts, dtype=torch.int64, device=self.device if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)          # also the barrier: every part file is closed before the merge
        counts = [int(x) for x in tot.cpu().tolist()]
        # join the parts (rank order = input order) concurrently: every rank copies its own part to the offset that the sizes
        # of the lower ranks' parts give; gzip parts are complete members, whose concatenation is a valid gzip file
        mine = [os.path.getsize(part_path(path, self.rank)) for path in finals]
        sizes = self._all_gather(mine)
        # the join goes into '<final>.joining' and is renamed after the last barrier: a run that dies while the parts are
        # being placed never leaves a full-size, partly zero-filled file under the final name
        tmps = [path + '.joining' for path in finals]
        self._part_files += tmps if self.rank == 0 else []
        # .gz files whose members were made on the device are BGZF: one end-of-file block (an empty member) behind the last part
        tails = [_gzmod.eof_block() if ((self.gzip_on_device and path.endswith('gz')) or (self.bam_files and path.endswith(('.bam', '.ubam'))))
                 else b'' for path in finals]
        if self.rank == 0:
            for f, tmp in enumerate(tmps):
                with open(tmp, 'wb') as fh:
                    body = sum(sz[f] for sz in sizes)
                    fh.truncate(body + len(tails[f]))
                    if tails[f]:
                        fh.seek(body)
                        fh.write(tails[f])
        dist.barrier()
        for f, path in enumerate(finals):
            fx.place_part(tmps[f], part_path(path, self.rank), sum(sizes[r][f] for r in range(self.rank)))
        dist.barrier()
        if self.rank == 0:
            for tmp, path in zip(tmps, finals):
                os.replace(tmp, path)
        self._part_files = []
        dist.barrier()
        return counts

    @staticmethod
    def gz_output_files(output, rrna, is_paired, ensure):
        """(mate, label) of every output file that is written gzip-compressed - by name, like the reference's writer
        (detect.py:738: read_file.endswith('gz')); the '<out>.unclassified.gz' files of --ensure both (detect.py:390-400) always are.
        The same list on every rank (it depends on the arguments only): the files whose records are deflated on the device."""
        # (one file per mate - or, for the pairs of an interleaved input, ONE file per label: its key is mate 0's)
        files = [(e, lab) for lab, names in ((1, rrna), (0, output)) if names is not None for e, name in enumerate(names)
                 if name.endswith('gz') or name.endswith(('.bam', '.ubam'))]      # (BAM names: --bam_output / --ubam_output only - BGZF members, like a .gz)
        if is_paired and ensure == 'both':
            files += [(e, -1) for e in range(len(output))]
        return files

    def _close_arenas(self):
        for a in self._arenas:
            a.close()
        self._arenas = []

    def run(self):
        """Whole-file mode of the reference (detect.py:121-324): same outputs; streamed here in 1 Mi-record chunks
        instead of holding the parsed file in host RAM."""
        self.run_with_chunks(chunk_reads=DEFAULT_CHUNK_READS)

    def detect(self):
        """Argument checks, batch-size rule, dispatch (reference detect.py:525-584)."""
        self.input = self.args.input
        self.output = self.args.output
        self.rrna = self.args.rrna
        self.pack_seq = self.config['arch']['args']['pack_seq']
        try:
            self.is_paired = check_file_counts(self.input, self.output, self.rrna, self.interleaved)
        except RuntimeError as e:
            self.logger.error('{}{}{}'.format(colors.FAIL, _COUNT_ERRORS.get(str(e), str(e)), colors.ENDC))
            raise
        check_read_report(self.report_path, self.output, self.rrna, self.is_paired, self.args.ensure, self.bam_files)
        check_summary(self.summary_path, self.output, self.rrna, self.is_paired, self.args.ensure, self.report_path, self.bam_files)
        check_read_groups(self.read_groups, self.summary_path, self.input, self.bam_shard)
        check_bam_tags(self.bam_tags_arg, self.input, self.bam_output, floats=self.bam_tag_floats)
        self._split_ids = check_split_groups(self.split_groups, self.input, self.output, self.rrna, self.args.ensure, self.report_path,
                                             self.summary_path, self.regions_path, self.bam_output, self.interleaved)
        self._windows = check_windows(self.args)
        check_regions(self.regions_path, self._windows is not None, self.output, self.rrna, self.is_paired, self.args.ensure,
                      self.report_path, self.summary_path, self.bam_files)
        # reference batch-size heuristic (detect.py:558-568); kept because --chunk_size is expressed in these batches
        denom = (2 * self.len * 6.4) if self.is_paired else (self.len * 6.4)
        self.batch_size = 2 ** math.floor(math.log2(((self.args.memory - 2) * 1024 * 1024) / denom))
        self.logger.info('Choose batch size: {}{}{}{} based on the given GPU RAM size {}GB and max read length {}'.format(
            colors.BOLD, colors.OKCYAN, self.batch_size, colors.ENDC, self.args.memory, self.len))
        if self.chunk_size is None:
            self.run()
        else:
            self.run_with_chunks()

    # ---- label helpers with the reference's signatures (host lists; used by tests / API users) -----------------
    @staticmethod
    def separate_reads(reads, labels):
        """{label: [reads]} (reference detect.py:600-614)"""
        out = {}
        for read, label in zip(reads, labels):
            out.setdefault(int(label), []).append(read)
        return out

    def separate_paired_reads(self, r1_reads, r1_outs, r2_reads, r2_outs):
        """Pair fusion on the device (rd_pair_fuse) then the reference's dict-of-lists result (detect.py:616-663)."""
        lab = module_arch.pair_fuse(r1_outs.contiguous(), r2_outs.contiguous(), self.args.ensure).cpu().tolist()
        return Predictor.separate_reads(r1_reads, lab), Predictor.separate_reads(r2_reads, lab)


_COUNT_ERRORS = {       # what the log says in front of the two file-count errors of the reference
    "Input or output should have no more than two files and they should have the same number of files.":
        "The number of input and output sequence files is invalid!",
    "Ouput rRNA should have no more than two files and they should the same number with input files.":
        "The number of output rRNA sequence files is invalid!"}


def check_file_counts(inputs, output, rrna, interleaved=False):
    """The rules for the numbers of -i / -o / -r files (reference detect.py:525-545); returns whether the run is paired-end. Raises
    RuntimeError. --interleaved: ONE FASTQ input whose records alternate mate 1, mate 2; one -o path (an interleaved output) or two
    (mate 1's records and mate 2's), and as many -r paths if any."""
    n_in, n_out = len(inputs or []), len(output or [])
    n_rrna = None if rrna is None else len(rrna)
    if interleaved:
        if n_in != 1:
            raise RuntimeError("--interleaved takes exactly one input file (-i), whose records alternate mate 1, mate 2; got {}".format(n_in))
        if fx.get_seq_format(inputs[0]).startswith("fa"):
            raise RuntimeError("--interleaved: interleaved FASTA is not supported (the input must be FASTQ)")
        if n_out not in (1, 2):
            raise RuntimeError("--interleaved takes one output file (-o: interleaved) or two (mate 1's and mate 2's records); got {}".format(n_out))
        if n_rrna is not None and n_rrna != n_out:
            raise RuntimeError("--interleaved: -r takes as many files as -o ({}); got {}".format(n_out, n_rrna))
        return True
    if n_in != n_out or n_in > 2 or n_in < 1:
        raise RuntimeError("Input or output should have no more than two files and they should have the same number of files.")
    if n_rrna is not None and n_rrna != n_in:
        raise RuntimeError("Ouput rRNA should have no more than two files and they should the same number with input files.")
    return n_in == 2


def unclassified_path(out, bam_output=False):
    """the file of the unclassified pairs (-e both) that goes with the -o file `out`: '<out>.unclassified.gz', or under --bam_output
    '<out>.unclassified.bam' - the one place that knows the name (the collision checks of --read_report / --summary / --regions use it)"""
    return out + ('.unclassified.bam' if bam_output else '.unclassified.gz')


def check_bam(inputs, output, rrna, bam_output=False, bam_shard=False, interleaved=False, ubam_output=False):
    """BAM input (.bam / .ubam, ribodetector_amd/bam.py): the rules that hold before anything touches a device; returns whether the
    inputs are BAM. The records become FASTQ text on the device, so the outputs are FASTQ files; there is no host reader for BAM,
    so the switches and layouts that need one are refused. bam_output (--bam_output): every input is BAM and every -o / -r name ends
    with .bam / .ubam - the selected records are written as they stand in the input (all outputs are BAM or none is). bam_shard
    (--bam_shard): BAM input under several ranks, each one with its own share of the records (data_loader/bam_shard.py) - the sharded
    parse of BGZF members, so not with RD_BGZF_SHARD=0, and not an interleaved file (no byte range of one holds whole pairs by itself).
    ubam_output (--ubam_output; check_ubam has its rules): .bam / .ubam names on -o / -r are what the run writes."""
    def fmt(path):
        try:
            return fx.get_seq_format(path)
        except ValueError:
            return None                          # (the run reports unknown extensions, as ever)
    outs = list(output or []) + list(rrna or [])
    kinds = [fmt(p) for p in inputs or []]
    if bam_output:
        if not kinds or any(k != "bam" for k in kinds):
            raise RuntimeError("--bam_output writes the records of BAM input as they stand: every -i file must end with .bam or .ubam, got {} "
                               "(checked before anything touches a device)".format(", ".join(str(p) for p in inputs or [])))
        for o in outs:
            if fmt(o) != "bam":
                raise RuntimeError("--bam_output: {} must end with .bam or .ubam - all outputs are BAM or none is (checked before anything "
                                   "touches a device)".format(o))
    for o in outs:
        if fmt(o) == "bam" and not (bam_output or ubam_output):
            raise RuntimeError("BAM output is not supported: {} (-o / -r take FASTQ names, plain or .gz; checked before anything touches a "
                               "device)".format(o))
    if "bam" not in kinds:
        if bam_shard:
            raise RuntimeError("--bam_shard shares BAM input between the ranks: every -i file must end with .bam or .ubam, got {} (checked "
                               "before anything touches a device)".format(", ".join(str(p) for p in inputs or [])))
        return False
    if any(k != "bam" for k in kinds):
        raise RuntimeError("BAM input cannot be mixed with FASTQ / FASTA input files: {} (checked before anything touches a "
                           "device)".format(", ".join(str(p) for p in inputs)))
    for o in outs:
        if not bam_output and fmt(o) not in ("fq", "fqgz"):
            raise RuntimeError("BAM input is written as FASTQ: {} must end with .fq or .fastq, plain or .gz (checked before anything "
                               "touches a device)".format(o))
    for name in ("RD_DEVICE_PARSE", "RD_DEVICE_INFLATE"):
        if fx.ingest_env(name, "1") == "0":
            raise RuntimeError("BAM input is framed and inflated on the device only: it cannot run with {}=0 or RD_INGEST=host (checked "
                               "before anything touches a device)".format(name))
    multi = int(os.environ.get("WORLD_SIZE", "1")) > 1
    if bam_shard and os.environ.get("RD_BGZF_SHARD", "1") == "0":
        raise RuntimeError("--bam_shard is the sharded parse of BGZF members: it cannot run with RD_BGZF_SHARD=0 (checked before anything "
                           "touches a device)")
    if bam_shard and interleaved and multi:
        raise RuntimeError("--bam_shard: an interleaved BAM is not shared by byte ranges: run on one rank (checked before anything touches "
                           "a device)")
    if multi and not bam_shard:
        raise RuntimeError("BAM input runs on one rank: the multi-rank layouts use the host reader, which has no BAM support (or give "
                           "--bam_shard; checked before anything touches a device)")
    return True


def check_ubam_tags(ubam_tags, ubam_output, floats=False):
    """--ubam_tags LIST (the BAM records of --ubam_output carry the listed tags of their header lines' comments;
    bam.tags_from_comment has the rule): only with --ubam_output, and a list that bam.parse_tag_list takes. Returns its names (2 bytes
    each, list order), or None without the flag. floats (--ubam_tag_floats) says what becomes of the float values of the listed tags,
    so it needs the list. Holds before anything touches a device."""
    if ubam_tags is None:
        if floats:
            raise RuntimeError("--ubam_tag_floats says how --ubam_tags reads float values: give --ubam_tags LIST with it "
                               "(checked before anything touches a device)")
        return None
    if not ubam_output:
        raise RuntimeError("--ubam_tags says which tags of the header lines' comments the BAM records of --ubam_output carry: give "
                           "--ubam_output with it (checked before anything touches a device)")
    return _ubammod.parse_list(ubam_tags)


def check_ubam(ubam_output, inputs, output, rrna, bam_output=False, parse_wanted=None, ubam_tags=None, ubam_tag_floats=False):
    """--ubam_output (FASTQ / FASTA input written as unaligned BAM; bam.from_fastq has the rule): the rules that hold before anything
    touches a device. The input is no BAM file (--bam_output writes those as they stand); not with --bam_output; every -o / -r name
    ends with .bam / .ubam (all outputs are BAM or none is); the chunks' text lives on the device, where the records are encoded - not
    RD_DEVICE_PARSE=0 or RD_INGEST=host, and no input that the device reader turns down (parse_wanted: device_reader.
    device_parse_wanted unless given); one rank. ubam_tags (--ubam_tags LIST: the records carry the listed tags of their header lines'
    comments, bam.tags_from_comment): only with --ubam_output, and a list that bam.parse_tag_list takes; returns its names, else None.
    ubam_tag_floats (--ubam_tag_floats): only with --ubam_tags."""
    tail = " (checked before anything touches a device)"
    names = check_ubam_tags(ubam_tags, ubam_output, ubam_tag_floats)
    if not ubam_output:
        return None

    def fmt(path):
        try:
            return fx.get_seq_format(path)
        except ValueError:
            return None
    if bam_output:
        raise RuntimeError("--ubam_output encodes FASTQ / FASTA input as BAM records, --bam_output writes the records of BAM input as they "
                           "stand: give one of them" + tail)
    for p in inputs or []:
        if fmt(p) == "bam":
            raise RuntimeError("--ubam_output takes FASTQ / FASTA input: {} is a BAM file, whose records --bam_output writes as they "
                               "stand".format(p) + tail)
    for o in list(output or []) + list(rrna or []):
        if fmt(o) != "bam":
            raise RuntimeError("--ubam_output: {} must end with .bam or .ubam - all outputs are BAM or none is".format(o) + tail)
    if fx.ingest_env("RD_DEVICE_PARSE", "1") == "0":
        raise RuntimeError("--ubam_output encodes the records where the chunks' text is, on the device: it cannot run with "
                           "RD_DEVICE_PARSE=0 or RD_INGEST=host" + tail)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("--ubam_output runs on one rank" + tail)
    wanted = dr.device_parse_wanted if parse_wanted is None else parse_wanted
    for p in inputs or []:
        if not wanted(p):
            raise RuntimeError("--ubam_output: the text of {} does not stay on the device (the device reader does not take this input "
                               "or the ingest switches keep it on the host)".format(p) + tail)
    return names


def check_read_report(path, output, rrna, is_paired, ensure, bam_output=False):
    """--read_report must not name a file the run writes anyway: an -o / -r file or an '<out>.unclassified.gz' file (-e both, pairs:
    one per -o path, also when the pairs come from one interleaved file)"""
    if not path:
        return
    same = lambda a, b: os.path.abspath(a) == os.path.abspath(b)      # noqa: E731
    for o in list(output or []) + list(rrna or []):
        if same(path, o):
            raise RuntimeError("--read_report {} is also an output sequence file (-o / -r)".format(path))
    if is_paired and ensure == 'both':
        for o in output or []:
            if same(path, unclassified_path(o, bam_output)):
                raise RuntimeError("--read_report {} is the unclassified pairs' output file".format(path))


def check_summary(path, output, rrna, is_paired, ensure, read_report=None, bam_output=False):
    """--summary must not name a file the run writes anyway: an -o / -r file, an '<out>.unclassified.gz' file (-e both, pairs) or the
    --read_report"""
    if not path:
        return
    taken = [(o, "an output sequence file (-o / -r)") for o in list(output or []) + list(rrna or [])]
    if is_paired and ensure == 'both':
        taken += [(unclassified_path(o, bam_output), "the unclassified pairs' output file") for o in output or []]
    if read_report:
        taken.append((read_report, "the --read_report file"))
    for o, what in taken:
        if os.path.abspath(path) == os.path.abspath(o):
            raise RuntimeError("--summary {} is also {}".format(path, what))


def check_bam_tags(bam_tags, inputs, bam_output=False, floats=False):
    """--bam_tags LIST: the rules that hold before anything touches a device; returns the listed names (2 bytes each, list order), or
    None without the flag. The list holds 1..16 names [A-Za-z][A-Za-z0-9], none twice (bamtags.parse_list); every input is BAM (the
    tags are those of BAM records); not with --bam_output, whose outputs keep every tag as it stands. floats (--bam_tag_floats) says
    how the float values of the listed tags are written, so it needs the list."""
    if bam_tags is None:
        if floats:
            raise RuntimeError("--bam_tag_floats says how --bam_tags writes float values: give --bam_tags LIST with it "
                               "(checked before anything touches a device)")
        return None
    names = _tagmod.parse_list(bam_tags)
    other = [p for p in inputs or [] if fx.get_seq_format(p) != "bam"]
    if other or not inputs:
        raise RuntimeError("--bam_tags copies the tags of BAM records into the FASTQ header lines: every -i file must end with .bam or .ubam, got {} "
                           "(checked before anything touches a device)".format(", ".join(other) or "no input"))
    if bam_output:
        raise RuntimeError("--bam_tags writes the tags into FASTQ header lines; with --bam_output the outputs are BAM files that keep every tag "
                           "already: give one of the two (checked before anything touches a device)")
    return names


def check_read_groups(read_groups, summary, inputs, bam_shard=False):
    """--read_groups: the rules that hold before anything touches a device; returns the declared groups of mate 1's BAM
    (bam.read_groups: [(id, fields)], header order), or None without the flag. The flag adds an object to the --summary file, so it
    needs one; the groups are those of BAM records and of a BAM header, so every input is BAM; the @RG lines of the header must be a
    dictionary (an ID each, none empty, none twice) of at most 65,536 groups. The header is read by the host's zlib."""
    if not read_groups:
        return None
    if not summary:
        raise RuntimeError("--read_groups adds the counters per read group to the --summary file: give --summary PATH too (checked before "
                           "anything touches a device)")

    def fmt(path):
        try:
            return fx.get_seq_format(path)
        except ValueError:
            return None
    if not inputs or any(fmt(p) != "bam" for p in inputs):
        raise RuntimeError("--read_groups counts the reads per RG tag of BAM records: every -i file must end with .bam or .ubam, got {} "
                           "(checked before anything touches a device)".format(", ".join(str(p) for p in inputs or [])))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not bam_shard:       # (--bam_shard: every rank counts its share, the rows are summed)
        raise RuntimeError("--read_groups runs on one rank (or give --bam_shard; checked before anything touches a device)")
    try:
        header = _bammod.header(inputs[0])
    except (OSError, ValueError) as e:
        raise RuntimeError("--read_groups: cannot read the header of {}: {} (checked before anything touches a device)".format(inputs[0], e))
    return _grpmod.check_groups(header)


SPLIT_FD_MARGIN = 64        # open files a run needs besides its outputs: inputs, libraries, the device, pipes


def split_families(output, rrna, paired_out, ensure, bam_output=False):
    """[(label, [path per mate])] of the output files of a run in the order _open_outputs opens them: -r, -o, and under -e both with
    pairs the unclassified files"""
    fams = ([(1, list(rrna))] if rrna else []) + [(0, list(output or []))]
    if paired_out and ensure == 'both':
        fams.append((-1, [unclassified_path(o, bam_output) for o in output or []]))
    return fams


def check_split_groups(split_groups, inputs, output, rrna, ensure, read_report=None, summary=None, regions=None, bam_output=False, interleaved=False):
    """--split_groups: the rules that hold before anything touches a device; returns the declared ids in the order of the device's
    rows (bam.sorted_ids), or None without the flag. Every output file becomes bam.split_paths(path, ids)."""
    if not split_groups:
        return None
    late = " (checked before anything touches a device)"

    def fmt(path):
        try:
            return fx.get_seq_format(path)
        except ValueError:
            return None
    if not inputs or any(fmt(p) != "bam" for p in inputs):
        raise RuntimeError("--split_groups writes one set of files per RG tag of BAM records: every -i file must end with .bam or .ubam, got {}{}".format(
            ", ".join(str(p) for p in inputs or []), late))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("--split_groups under several ranks is not implemented: run on one rank" + late)
    try:
        header = _bammod.header(inputs[0])
    except (OSError, ValueError) as e:
        raise RuntimeError("--split_groups: cannot read the header of {}: {}{}".format(inputs[0], e, late))
    try:
        groups = _bammod.read_groups(header)
    except ValueError as e:
        raise RuntimeError("--split_groups: {}{}".format(e, late))
    if len(groups) > _bammod.SPLIT_GROUPS_MAX:
        raise RuntimeError("--split_groups: the header declares {} read groups, more than {}{}".format(len(groups), _bammod.SPLIT_GROUPS_MAX, late))
    ids, _ = _bammod.sorted_ids([g[0] for g in groups])
    paired_out = len(inputs) == 2 or interleaved
    names = {}
    for what, path in (("--read_report", read_report), ("--summary", summary), ("--regions", regions)):
        if path:
            names.setdefault(os.path.abspath(path), []).append(what)
    n_files = 0
    for label, paths in split_families(output, rrna, paired_out, ensure, bam_output):
        for path in paths:
            if path.endswith('gz') and os.environ.get("RD_DEVICE_GZIP") == "host":
                raise RuntimeError("--split_groups: the members of {} are deflated on the device only: it cannot run with RD_DEVICE_GZIP=host "
                                   "(a host writer per file would hold a set of compressors per file){}".format(path, late))
            for member in _bammod.split_paths(path, ids):
                if len(os.fsencode(os.path.basename(member))) > 255:
                    raise RuntimeError("--split_groups: the file name {} is longer than 255 bytes{}".format(os.path.basename(member), late))
                names.setdefault(os.path.abspath(member), []).append(member)
                n_files += 1
    for key, who in names.items():
        if len(who) > 1:
            raise RuntimeError("--split_groups: two files of the run have the same name {}: {}{}".format(key, " and ".join(who), late))
    import resource
    soft = resource.getrlimit(resource.RLIMIT_NOFILE)[0]
    if soft != resource.RLIM_INFINITY and n_files + SPLIT_FD_MARGIN > soft:
        raise RuntimeError("--split_groups: the run writes {} files and needs {} open files, the limit is {}: raise it with ulimit -n{}".format(
            n_files, n_files + SPLIT_FD_MARGIN, soft, late))
    return ids


def check_windows(args):
    """--windows and its settings, checked before anything touches a device: None without the flag, else {"stride" (None = -l),
    "max_per_read", "fuse"}. RuntimeError for a setting without --windows, a stride outside 1..2^31-1 or more than 4096 (or fewer than
    1) windows per read."""
    stride, most, fuse = (getattr(args, k, None) for k in ('window_stride', 'max_windows', 'window_fuse'))
    if not getattr(args, 'windows', False):
        for flag, v in (('--window_stride', stride), ('--max_windows', most), ('--window_fuse', fuse)):
            if v is not None:
                raise RuntimeError("{} needs --windows".format(flag))
        return None
    if stride is not None and not 1 <= stride <= _winmod.STRIDE_MAX:
        raise RuntimeError("--window_stride must be in [1, 2^31 - 1]; got {}".format(stride))
    most = _winmod.DEFAULT_MAX_WINDOWS if most is None else most
    if not 1 <= most <= _native_mod.WINDOW_MAX:
        raise RuntimeError("--max_windows must be in [1, {}]; got {}".format(_native_mod.WINDOW_MAX, most))
    fuse = fuse or "mean"
    if fuse not in _native_mod.WINDOW_FUSE:
        raise RuntimeError("--window_fuse must be mean or max; got {!r}".format(fuse))
    return {"stride": stride, "max_per_read": int(most), "fuse": fuse}


def check_regions(path, windows, output=None, rrna=None, is_paired=False, ensure="none", read_report=None, summary=None, bam_output=False):
    """--regions needs --windows and must not name a file the run writes anyway: an -o / -r file, an '<out>.unclassified.gz' file (-e
    both, pairs), the --read_report or the --summary. Checked before anything touches a device."""
    if not path:
        return
    if not windows:
        raise RuntimeError("--regions needs --windows")
    taken = [(o, "an output sequence file (-o / -r)") for o in list(output or []) + list(rrna or [])]
    if is_paired and ensure == 'both':
        taken += [(unclassified_path(o, bam_output), "the unclassified pairs' output file") for o in output or []]
    taken += [(o, what) for o, what in ((read_report, "the --read_report file"), (summary, "the --summary file")) if o]
    for o, what in taken:
        if os.path.abspath(path) == os.path.abspath(o):
            raise RuntimeError("--regions {} is also {}".format(path, what))


def build_parser():
    args = argparse.ArgumentParser(description='rRNA sequence detector', formatter_class=RawTextHelpFormatter)
    args.add_argument('-c', '--config', default=None, type=str, help='Path of config file')
    args.add_argument('-d', '--deviceid', default=None, type=str,
                      help='Indices of GPUs to enable. Quotated comma-separated device ID numbers. (default: all)')
    args.add_argument('-l', '--len', type=int, required=True,
                      help='Sequencing read length. Note: the accuracy reduces for reads shorter than 40.')
    args.add_argument('-i', '--input', default=None, type=str, nargs='*', required=True,
                      help='Path of input sequence files (fasta and fastq), the second file will be considered as second end if two files given.\n'
                           '(extension) .bam / .ubam files are read too; their records are written as FASTQ.')
    args.add_argument('-o', '--output', default=None, type=str, nargs='*', required=True,
                      help='Path of the output sequence files after rRNAs removal (same number of files as input). \n(Note: 2 times slower to write gz files)')
    args.add_argument('-r', '--rrna', default=None, type=str, nargs='*',
                      help='Path of the output sequence file of detected rRNAs (same number of files as input)')
    args.add_argument('-e', '--ensure', default="none", type=str, choices=['rrna', 'norrna', 'both', 'none'],
                      help='''Ensure which classificaion has high confidence for paired end reads.
norrna: output only high confident non-rRNAs, the rest are clasified as rRNAs;
rrna: vice versa, only high confident rRNAs are classified as rRNA and the rest output as non-rRNAs;
both: both non-rRNA and rRNA prediction with high confidence;
none: give label based on the mean probability of read pair.
      (Only applicable for paired end reads, discard the read pair when their predicitons are discordant)''')
    args.add_argument('-t', '--threads', default=10, type=int, help='Number of threads to use. (default: 10)')
    args.add_argument('-m', '--memory', default=32, type=int, help='Amount (GB) of GPU RAM. (default: 12)')
    args.add_argument('--chunk_size', default=None, type=int,
                      help='Use this parameter when having low memory. Parsing the file in chunks.\n{}.\n{}.'.format(
                          'Not needed when free RAM >=5 * your_file_size (uncompressed, sum of paired ends)',
                          'When chunk_size=256, memory=16 it will load 256 * 16 * 1024 reads each chunk (use ~20 GB for 100bp paired end)'))
    args.add_argument('--log', default=None, type=str, help='Log file name')
    args.add_argument('--semantics', default=None, choices=['gpu', 'cpu'],
                      help='(extension) which reference product to reproduce for reads shorter than --len or ending in N:\n'
                           'gpu = ribodetector (packed sequences, default); cpu = ribodetector_cpu (zero-padded input).')
    args.add_argument('--read_report', default=None, type=str,
                      help='(extension) write one line per read (per pair for paired-end input) to this file, in input order:\n'
                           '  single-end: #read_id<TAB>label<TAB>p_rrna\n'
                           '  paired-end: #read_id<TAB>label<TAB>p_rrna_1<TAB>p_rrna_2<TAB>p_rrna_pair\n'
                           'read_id = the header up to its first whitespace (mate 1\'s for pairs); label = rRNA, nonrRNA or\n'
                           'unclassified (-e both), the output file the read went to; p_rrna = softmax of the final logits\n'
                           '(p_rrna_pair: of the summed logits of the mates, what decides -e none) as 0.dddd / 1.0000.\n'
                           'gzip-compressed when the name ends with gz.')
    args.add_argument('--summary', default=None, type=str,
                      help='(extension) write the run\'s QC counters to this file as JSON when the run has ended well: reads per label and\n'
                           'the rRNA fraction; per mate and label the histograms of read length, GC content and p_rrna (of each mate and\n'
                           'of the pair), the base composition; for pairs how often the mates agree. Counted on the GPU, chunk by chunk.')
    args.add_argument('--interleaved', action='store_true',
                      help='(extension) -i is ONE FASTQ file (plain or .gz) whose records alternate mate 1, mate 2: a paired-end run.\n'
                           '-o (and -r) take one path - interleaved output, the selected pairs in input order - or two: mate 1\'s\n'
                           'records and mate 2\'s, as for two input files. The ids of the two records of a pair (the header up to\n'
                           'its first whitespace) must be equal, or equal up to a trailing /1 and /2.')
    args.add_argument('--windows', action='store_true',
                      help='(extension) classify a read longer than -l over several windows of -l bases, spread evenly from its start to\n'
                           'its end, instead of its first -l bases alone; the windows\' logits are fused into one result per read.\n'
                           'Reads of at most -l bases are classified exactly as without the flag.')
    args.add_argument('--window_stride', default=None, type=int,
                      help='(extension) with --windows: a read of len bases gets ceil((len - l) / N) + 1 windows (default: -l, no overlap)')
    args.add_argument('--max_windows', default=None, type=int,
                      help='(extension) with --windows: the most windows per read, 1..4096 (default: 32); longer reads spread that many')
    args.add_argument('--window_fuse', default=None, type=str, choices=['mean', 'max'],
                      help='(extension) with --windows: mean = the mean of the windows\' logits (default); max = the logits of the window\n'
                           'with the largest rRNA margin ("rRNA if any stretch of the read is")')
    args.add_argument('--regions', default=None, type=str,
                      help='(extension) with --windows: write where the rRNA is inside the reads to this file, one line per region:\n'
                           '  #read_id<TAB>start<TAB>end<TAB>mate<TAB>windows<TAB>p_rrna_max\n'
                           'a region = a maximal run of consecutive windows of one read whose own logits say rRNA, as the interval\n'
                           '[start, end) in 0-based bases of that read; mate = 1 or 2 (read_id is that mate\'s); windows = the windows\n'
                           'of the run; p_rrna_max = the largest p_rrna among them. Independent of -e and --window_fuse.\n'
                           'gzip-compressed when the name ends with gz.')
    args.add_argument('--bam_output', action='store_true',
                      help='(extension) BAM input only: -o / -r take .bam / .ubam names, and every output file is a BAM file - the header of\n'
                           'its input and the selected records, byte for byte as they stand in the input (every tag kept), in input\n'
                           'order. Secondary / supplementary records are in no output. No @PG line is added.')
    args.add_argument('--ubam_output', action='store_true',
                      help='(extension) FASTQ / FASTA input, one rank: -o / -r take .bam / .ubam names, and every output file is an unaligned\n'
                           'BAM file of the selected records, encoded on the GPU: name = the header up to its first whitespace (in a\n'
                           'paired run without a trailing /1 of mate 1 or /2 of mate 2; empty: *), flag 4 / 77 / 141, bases as the\n'
                           'letters of =ACMGRSVTWYHKDBN in either case (U as T, anything else N), qualities clamped to 0..93 (FASTA:\n'
                           'absent), no tags. The header is @HD VN:1.6 SO:unsorted GO:query; no @PG line is added. A name of more\n'
                           'than 254 bytes ends the run with an error behind the chunks in front of it.')
    args.add_argument('--ubam_tags', default=None, type=str, metavar='LIST',
                      help='(extension) with --ubam_output: LIST = tag names separated by commas (MM,ML,RG; at most 16). Every BAM record\n'
                           'written carries the listed tags that the comment of its header line holds in SAM\'s text form -\n'
                           '@name<TAB>MM:Z:...<TAB>ML:B:C,... (what --bam_tags, samtools fastq -T and dorado --emit-fastq write) - in\n'
                           'comment order; an integer takes the smallest type that holds it. The comment is what stands behind the\n'
                           'one byte that ends the name, split at TABs; fields that are no tag (1:N:0:ACGT), tags that are not listed\n'
                           'and a listed name\'s second field are ignored. Float-typed values (f, B:f) are NOT copied; they are\n'
                           'counted (--ubam_tag_floats converts them). A record with a listed tag whose value is not what its type allows gets no tags and is\n'
                           'counted. Parsed and encoded on the GPU. The header stays @HD only: no @RG line is made up for RG:Z values.')
    args.add_argument('--ubam_tag_floats', action='store_true',
                      help='(extension) with --ubam_tags: a listed XY:f:value becomes a float32 tag and XY:B:f,value,... a float32 array\n'
                           'instead of being skipped: the float32 nearest to the exact decimal value, ties to even, denormals\n'
                           'included (12.5, .5, 1e-3, -inf, nan; no hex floats). A value that is no such number makes the record\n'
                           'malformed; one of more than 17 significant digits leaves its tag out and is counted. Converted on the\n'
                           'GPU in integer arithmetic.')
    args.add_argument('--read_groups', action='store_true',
                      help='(extension) BAM input with --summary: the summary gains "read_groups" - units (reads or pairs) and bases per\n'
                           'label for every @RG line of the header of the first -i file (by the records\' RG:Z tag; a pair counts in\n'
                           'mate 1\'s group), and for the records without RG, with an RG that no @RG line declares, and with malformed\n'
                           'tags. Counted on the GPU over the records as they stand in the input, which the run then keeps in GPU\n'
                           'memory next to the FASTQ text (about 0.75 of its bytes more).')
    args.add_argument('--split_groups', action='store_true',
                      help='(extension) BAM input, one rank: every output file becomes a family of files, one per @RG line of the header of\n'
                           'the first -i file and one for the rest: non.fq.gz -> non.rg-<id>.fq.gz ... and non.unassigned.fq.gz (bytes of an\n'
                           'id outside A-Z a-z 0-9 . _ + = @ , - are written %%XX). A read or pair goes to the member of MATE 1\'s RG:Z tag;\n'
                           'no RG, an undeclared value and malformed tags go to unassigned. Inside every file the records are in input\n'
                           'order and are the bytes the unsplit run writes. Every member is always written. Partitioned and deflated\n'
                           'on the GPU in one call per mate and chunk; the run keeps the records as they stand in the input in GPU memory.')
    args.add_argument('--bam_shard', action='store_true',
                      help='(extension) BAM input under several ranks (torch.distributed.run): every rank inflates, frames, classifies and\n'
                           'writes its own share of the records, like the ranks of a BGZF FASTQ run. The shares begin at record starts\n'
                           'found by a search on the GPU (8 records in a row that look like records); a cut that is none ends the run\n'
                           'with an error before any output is joined - run such a file on one rank. One rank: changes nothing.')
    args.add_argument('--bam_tags', default=None, type=str, metavar='LIST',
                      help='(extension) BAM input, FASTQ outputs: LIST = tag names separated by commas (MM,ML,RG; at most 16). Every FASTQ\n'
                           'record written carries the listed tags of its BAM record behind the read name, in list order, in SAM\'s\n'
                           'text form: @name<TAB>MM:Z:...<TAB>ML:B:C,... (what samtools fastq -T writes and minimap2 -y reads). A tag a\n'
                           'record does not have adds nothing. Float-typed values (f, B:f) are NOT copied; they are counted\n'
                           '(--bam_tag_floats writes them). A record whose listed tags are malformed, or hold a byte that no header\n'
                           'line may hold, gets no comment and is counted. Formatted on the GPU; the run keeps the records as they stand in the input and the tagged text in\n'
                           'GPU memory next to the FASTQ text. Not with --bam_output, which keeps every tag already.')
    args.add_argument('--bam_tag_floats', action='store_true',
                      help='(extension) with --bam_tags: a listed tag of type f is written as TG:f:value and a B:f array as\n'
                           'TG:B:f,value,... instead of being skipped, value = what printf("%%g") prints (6 significant digits of the\n'
                           'exact float32, ties to even). Formatted on the GPU in integer arithmetic.')
    args.add_argument('--no_mate_check', action='store_true', help='(extension) with --interleaved: do not compare the ids of the mates')
    args.add_argument('-v', '--version', action='version', version='%(prog)s {version}'.format(version=__version__))
    return args


def main(argv=None, log_level=None):
    args = build_parser().parse_args(argv)
    config_file = os.path.join(cd, 'config.json') if args.config is None else args.config
    config = ConfigParser.from_json(config_file)
    check_windows(args)                          # (before the model is loaded: nothing has touched a device yet)
    check_regions(args.regions, args.windows)    # (args is the parser's own Namespace: every option is there)
    # (in front of check_bam: several ranks are refused for the split as such, with or without --bam_shard)
    check_split_groups(args.split_groups, args.input, args.output, args.rrna, args.ensure, args.read_report, args.summary, args.regions,
                       args.bam_output, args.interleaved)
    check_ubam(args.ubam_output, args.input, args.output, args.rrna, args.bam_output, ubam_tags=args.ubam_tags, ubam_tag_floats=args.ubam_tag_floats)
    check_bam(args.input, args.output, args.rrna, args.bam_output, args.bam_shard, args.interleaved, ubam_output=args.ubam_output)
    check_read_groups(args.read_groups, args.summary, args.input, args.bam_shard)
    check_bam_tags(args.bam_tags, args.input, args.bam_output, floats=args.bam_tag_floats)
    seq_pred = Predictor(config, args, log_level=log_level)
    try:
        t0 = time.perf_counter()
        seq_pred.load_model()
        t1 = time.perf_counter()
        seq_pred.detect()
        t2 = time.perf_counter()
        fc = getattr(seq_pred, "_first_chunk", None)      # (time its labels arrived, its records): the rate after the pipeline filled
        steady = None
        if fc is not None and seq_pred.num_read > fc[1] and t2 > fc[0]:
            steady = (2 if seq_pred.is_paired else 1) * (seq_pred.num_read - fc[1]) / (t2 - fc[0])
        seq_pred.timing = {"load_model_s": t1 - t0, "detect_s": t2 - t1, "prefix_k": seq_pred.model.prefix_k,
                           "reads_per_s_after_first_chunk": steady, "ingest": getattr(seq_pred, "ingest", None),
                           "gz_ranges_s": getattr(seq_pred, "gz_shard_s", None), "pinned_cpus": getattr(seq_pred, "pinned_cpus", None),
                           "first_chunks_timeline": getattr(seq_pred, "_timeline", None), "run_started_at": getattr(seq_pred, "_t_run", None)}
        if os.environ.get("RD_TIMING_OUT"):          # (tools/host_scaling.py, tools/scale_sweep.sh: what a torchrun child measured, per rank)
            import json
            with open("%s.rank%d" % (os.environ["RD_TIMING_OUT"], seq_pred.rank), "w") as fh:
                json.dump(dict(seq_pred.timing, rank=seq_pred.rank, world=seq_pred.world, num_read=seq_pred.num_read,
                               thread_cpu_s=seq_pred.thread_cpu_s, process_cpu_s=time.process_time(), main_thread_s=getattr(seq_pred, "_stage_s", None),
                               phases_s=getattr(seq_pred, "phases_s", None)), fh, default=str)
    except BaseException:
        seq_pred.cleanup()                       # a failed run leaves no slot, '<out>.partN' or '<out>.joining' files behind
        if seq_pred.multi:
            # a rank that fails must not leave the others waiting in a collective (and must not wait in one itself while the
            # interpreter shuts down): report and leave at once - torch.distributed.run then tears the other ranks down
            import sys
            import traceback
            traceback.print_exc()
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(1)
        raise
    return seq_pred


if __name__ == '__main__':
    main()
