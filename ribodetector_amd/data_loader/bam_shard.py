"""A BAM file shared by the ranks of a run (detect.py --bam_shard): BamView gives fastx_parser.plan_ranges the four answers it asks
of an input - size, find_record_start, count_records, skip_records - for the inflated stream of a BAM file, so that the sharded-parse
layout of BGZF FASTQ carries BAM as it stands: rank 0 indexes the members, every rank inflates, frames, classifies and writes its share.

BAM records are a length-prefixed chain without a delimiter; "the first record start at or behind offset p" is answered by a search
(the rule: bam.find_record_start; on the device: C ABI rd_bam_find_start, csrc/rd_bam_shard.hpp) over a probe of inflated bytes
behind p, which grows while the answer is undecided. The answer is a record start unless the bytes imitate bam.CONFIRM records in a
row; a cut that is none is found out before any output is joined: count_records demands that the chain from a share's
start lands exactly on its end, and so does the feeder of the rank in front at run time.

device=None: zlib and the rule in Python (the CPU tests; a machine without a GPU). Positions are offsets into the inflated stream."""
import ctypes as C
import struct

import numpy as np

from .. import _native as N
from .. import bam
from . import fastx_parser as fx

_DEFAULT = object()


class BamView(fx.BgzfView):
    PROBE = 1 << 20            # inflated bytes behind the asked offset that find_record_start looks at first; fourfold while undecided
    PROBE_MAX = 256 << 20
    BATCH = 32 << 20           # compressed bytes per batch of count_records on the device
    WINDOW = 1 << 20           # inflated bytes per window of the walks on the host (skip_records; count_records without a device)

    def __init__(self, path, index=None, header_len=None, device=_DEFAULT):
        """index: fx.BgzfView.build_index(path) (rank 0 builds it, the others receive it); header_len: bam.header_bytes(path);
        device: where the probes and shares are inflated and searched - default: the current GPU if there is one; None: the host"""
        super().__init__(path, index=index, fasta=False)
        self.header_len = int(bam.header_bytes(self.path) if header_len is None else header_len)
        if device is _DEFAULT:
            import torch
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        self.device = device
        self._dg = None
        self._wb, self._w = 0, b""
        self.stats = {"probes": 0, "probe_bytes": 0, "count_batches": 0}

    # ---- inflated bytes ----------------------------------------------------------------------------------------------------------
    def _bytes(self, p, n):
        """text(p, p + n) out of a cached window (host walks)"""
        if not (self._wb <= p and p + n <= self._wb + len(self._w)):
            self._wb, self._w = p, self.text(p, p + max(n, self.WINDOW))
        return self._w[p - self._wb:p - self._wb + n]

    def _gunzip(self):
        if self._dg is None:
            from .. import gz
            self._dg = gz.DeviceGunzip(self.device)
        return self._dg

    def _inflate(self, fh, m, e, text_out=None):
        """the members [m, e) inflated on the device: (uint8 tensor of their text - text_out[:n] if given -, n)"""
        dg = self._gunzip()
        c0 = max(0, int(self.comp_off[m]) - 64)                # (64: bytes read in front of a member's DEFLATE data - its gzip header)
        c1 = int(self.comp_off[e - 1]) + int(self.comp_len[e - 1]) + 8
        fh.seek(c0)
        buf = np.frombuffer(fh.read(c1 - c0), dtype=np.uint8).copy()
        tab = np.zeros((e - m, 3), dtype=np.int64)             # the member table of this batch, from the index (rd_gz_member's layout)
        tab[:, 0] = self.comp_off[m:e] - c0
        tab[:, 1] = self.out_off[m:e] - self.out_off[m]
        tab[:, 2] = self.comp_len[m:e] | ((self.out_off[m + 1:e + 1] - self.out_off[m:e]) << 32)
        dg.set_members(tab)
        ob = int(self.out_off[e] - self.out_off[m])
        if text_out is None:
            return dg.inflate(buf, len(buf), e - m, ob), ob
        dg.submit(buf, len(buf), e - m, ob, slot=0, text_out=text_out)
        dg.finish(0)
        return text_out[:ob], ob

    # ---- the four answers ----------------------------------------------------------------------------------------------------------
    def find_record_start(self, pos):
        pos = int(pos)
        if pos <= self.header_len:
            return self.header_len
        if pos >= self.size:
            return self.size
        m0 = self._member_of(pos)
        base = int(self.out_off[m0])
        probe = self.PROBE
        while True:
            m1 = self._member_of(min(self.size, pos + probe) - 1) + 1          # whole members: [base, wend) holds [pos, pos + probe)
            wend = int(self.out_off[m1])
            at_eof = wend == self.size
            found, undecided = self._search(m0, m1, pos - base, wend - base, at_eof)
            self.stats["probes"] += 1
            self.stats["probe_bytes"] += wend - base
            if found >= 0 and (undecided < 0 or undecided > found):
                return base + found
            if at_eof and found < 0 and undecided < 0:         # pos lies inside the last record: no record starts behind it
                return self.size
            if at_eof or probe >= self.PROBE_MAX:
                raise ValueError(bam.NO_START % (wend - pos, pos, self.path))
            probe *= 4

    def _search(self, m0, m1, lo, end, at_eof):
        if self.device is None:
            base = int(self.out_off[m0])
            return bam.find_record_start(self.text(base, base + end), lo, end, at_eof)
        import torch
        with torch.cuda.device(self.device), open(self.path, "rb") as fh:
            text, n = self._inflate(fh, m0, m1)
            dg = self._gunzip()
            with torch.cuda.stream(dg.stream):
                info = torch.empty(4, dtype=torch.int64, device=self.device)
                N.check(N.lib().rd_bam_find_start(N.ptr(text), lo, end, end, 1 if at_eof else 0, N.ptr(info), C.c_void_p(dg.stream.cuda_stream)),
                        "rd_bam_find_start")
                info = info.cpu()
            if int(info[3]):
                raise RuntimeError("rd_bam_find_start: bad arguments (%d, %d, %d)" % (lo, end, end))
            return int(info[0]), int(info[1])

    def skip_records(self, start, k):
        """the offset just behind the k-th delivered record (flag & 0x900: not delivered) from `start`, a record start; k = 0: start"""
        p, k = int(start), int(k)
        if k <= 0:
            return p
        p = max(p, self.header_len)
        for q, size, flag in self._walk(p, self.size):
            if not flag & bam.SKIP_FLAGS:
                k -= 1
                if k == 0:
                    return q + size
        return self.size

    def _walk(self, a, b):
        """(offset, bytes with the block_size field, flag) of the records of the chain from a that start in front of b: the walk of
        bam.records over windows of the stream, by zlib. ValueError where that walk raises one (record numbers count from a)."""
        p, k = a, 0
        while p < b:
            if self.size - p < 4:
                raise ValueError(bam.TRUNCATED)
            block = struct.unpack_from("<i", self._bytes(p, 4))[0]
            if block < 32:
                raise ValueError(bam.MALFORMED % k)
            if p + 4 + block > self.size:
                raise ValueError(bam.TRUNCATED)
            f = self._bytes(p, 36)
            l_name, n_cigar, flag, l_seq = f[12], struct.unpack_from("<H", f, 16)[0], struct.unpack_from("<H", f, 18)[0], struct.unpack_from("<I", f, 20)[0]
            if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > block or l_name < 1 or self._bytes(p + 36 + l_name - 1, 1) != b"\0":
                raise ValueError(bam.MALFORMED % k)
            yield p, 4 + block, flag
            p += 4 + block
            k += 1

    def count_records(self, start, end):
        """the delivered records of the share [start, end); start is a record start (or lies in the header: the header's end). The chain
        from `start` must land exactly on `end`: ValueError(bam.NOT_A_BOUNDARY) if it does not and `end` is not the file's end"""
        a, b = max(int(start), self.header_len), min(self.size, int(end))
        if b <= a:
            return 0
        try:
            n, landed = self._count_host(a, b) if self.device is None else self._count_device(a, b)
        except ValueError:
            if b < self.size:
                raise ValueError(bam.NOT_A_BOUNDARY % (b, self.path, bam.CONFIRM)) from None
            raise
        if not landed:
            raise ValueError(bam.NOT_A_BOUNDARY % (b, self.path, bam.CONFIRM))
        return n

    def _count_host(self, a, b):
        n, p = 0, a
        for q, size, flag in self._walk(a, b):
            n += 0 if flag & bam.SKIP_FLAGS else 1
            p = q + size
        return n, p == b

    def _count_device(self, a, b):
        """the share inflated in batches of members and walked where it lands (rd_bam_count: the carry chains the batches)"""
        import torch
        lib = N.lib()
        m, m1 = self._member_of(a), self._member_of(b - 1) + 1
        n, walked, prev, landed = 0, 0, None, False
        with torch.cuda.device(self.device), open(self.path, "rb") as fh:
            dg = self._gunzip()
            sp = C.c_void_p(dg.stream.cuda_stream)
            carry = 0
            while m < m1:
                e = min(m1, max(m + 1, int(np.searchsorted(self.comp_off, self.comp_off[m] + self.BATCH))))
                ob = int(self.out_off[e] - self.out_off[m])
                pad = ((carry + 63) // 64) * 64                                 # room in front of the new bytes for the carry of the batch before
                with torch.cuda.stream(dg.stream):
                    text = torch.empty(((pad + ob + 64 + 127) // 64) * 64, dtype=torch.uint8, device=self.device)
                    summary = torch.zeros(8, dtype=torch.int64, device=self.device)
                self._inflate(fh, m, e, text_out=text[pad:pad + ob])
                lo = pad + max(a, int(self.out_off[m])) - int(self.out_off[m])
                hi = pad + min(b, int(self.out_off[e])) - int(self.out_off[m])
                final = e == m1
                with torch.cuda.stream(dg.stream):
                    ws = torch.empty(max(int(lib.rd_bam_count_workspace_bytes(hi)), 256), dtype=torch.uint8, device=self.device)
                    N.check(lib.rd_bam_count(N.ptr(text), lo, hi, N.ptr(prev[0]) if prev else None, N.ptr(prev[1]) if prev else None, 1 if final else 0,
                                             N.ptr(summary), N.ptr(ws), ws.numel(), sp), "rd_bam_count")
                    h = summary.cpu().numpy()
                self.stats["count_batches"] += 1
                status = int(h[6]) & 0xffffffff
                if status == N.BAM_RECORD:
                    raise ValueError(bam.MALFORMED % (walked + int(h[5])))
                if status == N.BAM_TRUNCATED:
                    raise ValueError(bam.TRUNCATED)
                if status:
                    raise RuntimeError("rd_bam_count: status %d" % status)
                n += int(h[3])
                walked += int(h[2])
                carry = int(h[1] - h[4])                                        # end - consumed
                landed = carry == 0
                prev = (text, summary)
                m = e
        return n, landed
