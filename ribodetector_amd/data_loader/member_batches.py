"""A BGZF file as batches of whole gzip members for the device member decoder - the ONE producer loop of the two feeders
(fastx_parser._DeviceInflateFeeder: the text comes back to the host parser; device_reader.DeviceFeeder: the text stays in HBM) - and
the zlib tail both fall back to where the members stop carrying their size. Nothing here touches the GPU: no torch, no gz.py - the
feeders pass `index` (gz.DeviceGunzip.index), their slot queue and numpy views of their pinned buffers."""
import os
import time
import zlib
from collections import namedtuple

TRUNCATED = "Compressed file ended before the end-of-stream marker was reached"      # (Python's gzip module's words: tests match on them)

# a batch with members, whose slot the consumer now owns: bufs[slot][:nbytes] holds n whole members that inflate to out_bytes bytes, of
# which [drop, drop + take) are the share's (everything unless a span was given)
Batch = namedtuple("Batch", "slot nbytes n out_bytes drop take")
# the last event of a file whose members stop carrying their size: the bytes read but not consumed, for zlib_member_texts(fh, data)
Tail = namedtuple("Tail", "data")


def error_bytes(e):
    """an exception as the reader's error text (rd_reader_feed_end)"""
    return (str(e) or repr(e)).encode()[:400]


def skip_zero_padding(fd, pos, size):
    """the offset of the first non-zero byte at or behind pos (size: none) - zero padding behind a member is skipped, as Python's gzip module does"""
    while pos < size:
        rest = os.pread(fd, 1 << 16, pos)
        k = len(rest) - len(rest.lstrip(b"\0"))
        pos += k
        if k < len(rest):
            break
    return pos


def pread_exactly(fd, view, valid, pos):
    """view[:valid] = the file's bytes [pos, pos + valid), or ValueError"""
    have = 0
    while have < valid:
        k = os.preadv(fd, [memoryview(view)[have:valid]], pos + have)
        if k <= 0:
            raise ValueError(TRUNCATED)
        have += k


def member_batches(fh, index, acquire, release, bufs, first, full, span=None, slack=1 << 20, stopped=lambda: False, tm=None):
    """fh: the file, unbuffered. index(buf, have, slot) -> (n, consumed, out_bytes, streaming). acquire() -> a free slot (blocking; None:
    stopped), release(slot) gives back one that carried nothing; bufs[slot]: full + slack bytes. Batches of `first` compressed bytes,
    doubling up to `full`. span = (first file byte, one past the last, text bytes to drop in front, text bytes to deliver): a rank's
    share (BgzfView.file_span). tm: seconds are added to its "wait_slot", "read" and "index". Yields Batch events and at most one Tail."""
    carry = None                                    # bytes of an incomplete member, to go in front of the next batch
    batch = min(first, full)
    eof = False
    file_left = text_left = None
    skip_text = 0
    if span is not None:                            # a share of the file: whole members [c0, c1), text trimmed at both ends
        fh.seek(span[0])
        file_left, skip_text, text_left = span[1] - span[0], span[2], span[3]
        eof = file_left <= 0
    while not stopped():
        t0 = time.perf_counter()
        slot = acquire()                            # (its previous batch has left the GPU)
        if slot is None:
            return
        t1 = time.perf_counter()
        buf, have = bufs[slot], 0
        if carry is not None:
            have = len(carry)
            buf[:have] = carry
            carry = None
        while have < batch and not eof:
            cap = batch + slack if file_left is None else min(batch + slack, have + file_left)
            k = fh.readinto(memoryview(buf)[have:cap])
            if not k:
                eof = True
            else:
                have += k
                if file_left is not None:
                    file_left -= k
                    eof = file_left <= 0
        if have == 0:
            release(slot)
            return
        t2 = time.perf_counter()
        n, consumed, out_bytes, streaming = index(buf, have, slot)
        if tm is not None:
            tm["wait_slot"] += t1 - t0
            tm["read"] += t2 - t1
            tm["index"] += time.perf_counter() - t2
        if streaming and n == 0:
            # a member without a size subfield behind the BGZF blocks (`cat a.bgzf.gz b.gz` is a legal .gz): the rest of the file is
            # for zlib on the host, behind the batches in flight
            rest = bytes(buf[consumed:have])
            release(slot)
            yield Tail(rest)
            return
        if (n == 0 or consumed == 0) and eof:
            release(slot)
            if consumed < have:
                raise ValueError(TRUNCATED)
            return
        if consumed == 0 and have >= full:          # a member that claims to be larger than the batch buffer: the loop would spin
            release(slot)
            raise ValueError("gzip member larger than %d bytes: not a BGZF file (RD_DEVICE_INFLATE=0 reads it with the host's decoders)" % full)
        if consumed < have:
            carry = buf[consumed:have].copy()
        if n:
            drop, take = 0, out_bytes
            if text_left is not None:
                drop = min(skip_text, out_bytes)
                take = min(out_bytes - drop, text_left)
                skip_text -= drop
                text_left -= take
            yield Batch(slot, consumed, n, out_bytes, drop, take)
        else:
            release(slot)
        batch = min(2 * batch, full)
        if text_left is not None and text_left <= 0:
            return


def zlib_member_texts(fh, data, stopped=lambda: False):
    """the text of the gzip members in `data` + the rest of fh (a file whose members stop carrying their size), by zlib, member after
    member: bytes of at most 16 MiB. Zero padding behind a member is dropped (Python's gzip module skips it too)."""
    d, inside = zlib.decompressobj(31), False
    while not stopped():
        if not data:
            data = fh.read(4 << 20)
            if not data:
                if inside:
                    raise ValueError(TRUNCATED)
                return
        if not inside and not data.strip(b"\0"):
            data = b""
            continue
        try:
            out = d.decompress(data, 16 << 20)
        except zlib.error as e:
            raise ValueError(str(e))
        inside = True
        if out:
            yield out
        if d.eof:
            data, d, inside = d.unused_data, zlib.decompressobj(31), False
        else:
            data = d.unconsumed_tail
