"""Plain numpy statements of what the reference-layout encoders and the label kernels must produce (include/ribodetector_amd.h:
rd_encode_codes, rd_encode_onehot_padded, rd_pack_plan, rd_pack_onehot, rd_pair_fuse, rd_count_labels), written from the
reference's behaviour (seq_encoder.py:11-18,126-145, detect.py:616-689) and not from the kernels. Test helper: numpy only, no GPU,
no native code. tests/test_encoder_truth_host.py holds every function here to the CPU oracle, the golden fixtures and torch."""
import numpy as np

LUT = np.full(256, 4, dtype=np.uint8)          # A C G T U(=T) -> 0 1 2 3; every other byte, lower case included -> 4
for _ch, _c in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"U", 3)):
    LUT[_ch[0]] = _c
ONEHOT = np.concatenate([np.eye(4, dtype=np.float32), np.zeros((1, 4), dtype=np.float32)])    # code 4 = the zero row


def steps(lens, max_len):
    """T = clip(len, 0, max_len): the bases of a read that count"""
    return np.clip(np.asarray(lens, dtype=np.int64), 0, int(max_len))


def codes(arena, off, lens, max_len, stride=None):
    """uint8 [n, stride]: the code of base t of read i for t < T, 4 from there on"""
    stride = int(max_len if stride is None else stride)
    arena = np.asarray(arena, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)[:len(lens)]
    T = steps(lens, max_len)
    pos = np.arange(stride, dtype=np.int64)
    valid = pos[None, :] < T[:, None]
    at = np.where(valid, off[:, None] + pos[None, :], 0)
    return np.where(valid, LUT[arena[at]], np.uint8(4)).astype(np.uint8)


def padded(arena, off, lens, max_len):
    """float32 [n, max_len, 4]: one-hot rows, zero rows for other bytes and past T"""
    return ONEHOT[codes(arena, off, lens, max_len)]


def pack_plan(lens, max_len):
    """(sorted int64[n], unsorted int64[n], batch_sizes int64[max_len], total): pack_sequence(enforce_sorted=False) of the
    truncated reads, ties in input order"""
    T = steps(lens, max_len)
    order = np.argsort(-T, kind="stable").astype(np.int64)
    inverse = np.empty_like(order)
    inverse[order] = np.arange(len(T), dtype=np.int64)
    per_len = np.bincount(T, minlength=int(max_len) + 1)             # reads of each T
    longer = len(T) - np.cumsum(per_len)                              # longer[t] = reads with T > t
    return order, inverse, longer[:int(max_len)].astype(np.int64), int(T.sum())


def pack_data(arena, off, lens, max_len):
    """float32 [total, 4]: PackedSequence.data, timestep-major over the sorted reads"""
    order = pack_plan(lens, max_len)[0]
    T = steps(lens, max_len)[order]
    c = codes(arena, np.asarray(off, dtype=np.int64)[:len(lens)][order], np.asarray(lens)[order], max_len)
    alive = np.arange(int(max_len))[:, None] < T[None, :]             # [t, j]
    return ONEHOT[c.T[alive]]


def pair_fuse(l1, l2, mode):
    """int8 [n] from the mates' logits float32 [n, 2]: the pair label of detect.py:616-663"""
    l1 = np.asarray(l1, dtype=np.float32).reshape(-1, 2)
    l2 = np.asarray(l2, dtype=np.float32).reshape(-1, 2)
    la, lb = l1[:, 1] > l1[:, 0], l2[:, 1] > l2[:, 0]
    if mode == "rrna":
        out = la & lb
    elif mode == "norrna":
        out = la | lb
    elif mode == "both":
        out = np.where(la == lb, la.astype(np.int8), np.int8(-1))
    elif mode == "none":
        with np.errstate(invalid="ignore", over="ignore"):
            s0 = (l1[:, 0] + l2[:, 0]).astype(np.float32)
            s1 = (l1[:, 1] + l2[:, 1]).astype(np.float32)
        out = s1 > s0
    else:
        raise ValueError(mode)
    return out.astype(np.int8)


def count(labels):
    """(labels equal to 0, labels equal to 1) of a uint8 array; every other value counts nowhere"""
    lab = np.asarray(labels)
    assert lab.dtype == np.uint8
    return int(np.count_nonzero(lab == 0)), int(np.count_nonzero(lab == 1))


def fuse_counts(labels):
    """the three counters of rd_pair_fuse for its int8 labels: (0, 1, -1)"""
    lab = np.asarray(labels)
    return [int(np.count_nonzero(lab == 0)), int(np.count_nonzero(lab == 1)), int(np.count_nonzero(lab < 0))]
