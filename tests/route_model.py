"""Pure-numpy reference of the multi-GPU routing operations (include/rl_engine.h, the
rl_route_* entry points and the owner directory). No torch, no device; of rl_amd only
owner_of / mix64. Every function is the few-line definition the header states; the GPU tests
(tests/test_gpu_route_kernels.py) hold each kernel to it and tests/test_route_model.py holds it
to test_router_gloo.HostOps, the CPU stand-in the Python router runs on.

Packed results and return buffers are uint8 arrays (little-endian words, as on the device)."""
import numpy as np

import rl_amd

NS = 1_000_000
REMAINING_ERROR = -3                     # RL_REMAINING_ERROR
ESCAPE = 1                               # packed code of (allowed 1, remaining -3): never emitted
MAX_SHARDS = 64
_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


# ---------------------------------------------------------------- owners and the partition
def owners(keys, shards, dir_keys=None, dir_owner=None):
    """Owner shard of every key: the directory's where the key is listed (distinct keys),
    else the top log2(shards) bits of mix64(key)."""
    keys = np.asarray(keys, np.uint64)
    own = rl_amd.owner_of(keys, shards).astype(np.uint32)
    if dir_keys is not None and len(dir_keys) and keys.size:
        dk = np.asarray(dir_keys, np.uint64)
        order = np.argsort(dk, kind="stable")
        sk, so = dk[order], np.asarray(dir_owner, np.uint32)[order]
        pos = np.minimum(np.searchsorted(sk, keys), len(sk) - 1)
        hit = sk[pos] == keys
        own[hit] = so[pos[hit]]
    return own


def partition(own, skip=None, shards=None):
    """(perm, counts): perm = the requests with skip == 0 (skip None: all) in stable owner
    order, counts[s] = how many of them shard s owns."""
    own = np.asarray(own, np.uint32)
    live = np.arange(own.size) if skip is None else np.nonzero(np.asarray(skip) == 0)[0]
    perm = live[np.argsort(own[live], kind="stable")].astype(np.uint32)
    if shards is None:
        shards = int(own.max()) + 1 if own.size else 1
    return perm, np.bincount(own[live], minlength=shards).astype(np.int64)


def pack(perm, *cols):
    """rl_route_pack: every column gathered through perm (a None column: zeros of uint16)."""
    perm = np.asarray(perm, np.uint32)
    return tuple(np.zeros(perm.size, np.uint16) if c is None else np.asarray(c)[perm] for c in cols)


# ---------------------------------------------------------------- the int64 fold (wide path)
def fold(allowed, remaining):
    """packed = remaining * 2 + (allowed & 1), one int64 per decision."""
    return (np.asarray(remaining, np.int64) << 1) | (np.asarray(allowed, np.uint8) & 1).astype(np.int64)


def unfold(packed):
    packed = np.asarray(packed, np.int64)
    return (packed & 1).astype(np.uint8), packed >> 1


def scatter(perm, n, *cols):
    """out[perm[j]] = col[j] for every column; entries perm does not name stay 0."""
    outs = []
    for c in cols:
        c = np.asarray(c)
        o = np.zeros(n, c.dtype)
        o[np.asarray(perm, np.uint32)[:c.size]] = c
        outs.append(o)
    return tuple(outs)


# ---------------------------------------------------------------- packed widths
def width_hi(w):
    """The largest remaining a w-byte packed result holds."""
    return ((2 ** (8 * w) - 1) >> 1) - 3


def fits(remaining, w):
    remaining = np.asarray(remaining, np.int64)
    return (remaining >= -3) & (remaining <= width_hi(w))


def _pack_words(allowed, remaining, w):
    v = ((np.asarray(remaining, np.int64) + 3).astype(np.uint64) << np.uint64(1)) | \
        (np.asarray(allowed, np.uint8) & 1).astype(np.uint64)
    return v.astype(_U[w])                                       # truncation to w bytes


def fold_packed(allowed, remaining, w):
    """(remaining + 3) << 1 | (allowed & 1) in w little-endian bytes each. Exact on
    remaining in [-3, width_hi(w)] without the pair (allowed 1, remaining -3)."""
    return np.ascontiguousarray(_pack_words(allowed, remaining, w)).view(np.uint8).copy()


def unfold_packed(data, w):
    v = np.ascontiguousarray(np.asarray(data, np.uint8)).view(_U[w]).astype(np.uint64)
    return (v & np.uint64(1)).astype(np.uint8), (v >> np.uint64(1)).astype(np.int64) - 3


# ---------------------------------------------------------------- segmented return trip
def ret_layout(seg_counts, w, cap):
    """(segment offsets, exception-block offsets, total bytes): every segment is its packed
    results padded to 8 B, then {u64 count, cap x (i64 position, i64 remaining)}."""
    seg, blk, o = [], [], 0
    for c in seg_counts:
        c = int(c)
        seg.append(o)
        o += (c * w + 7) // 8 * 8
        blk.append(o)
        o += 8 + 16 * int(cap)
    return seg, blk, o


def return_bytes(seg_counts, w, cap):
    """rl_route_return_bytes, bad arguments included (0)."""
    if len(seg_counts) == 0 or len(seg_counts) > MAX_SHARDS or w not in _U:
        return 0
    return ret_layout(seg_counts, w, cap)[2]


def fold_return(allowed, remaining, seg_counts, w):
    """Per segment: (packed bytes, set of (position in the segment, remaining) escapes). An
    escape is a remaining outside [-3, width_hi(w)]; its packed word is ESCAPE."""
    allowed = np.asarray(allowed, np.uint8)
    remaining = np.asarray(remaining, np.int64)
    out, beg = [], 0
    for c in seg_counts:
        c = int(c)
        a, r = allowed[beg:beg + c], remaining[beg:beg + c]
        ok = fits(r, w)
        words = np.where(ok, _pack_words(a, np.where(ok, r, 0), w), ESCAPE).astype(_U[w])
        esc = np.nonzero(~ok)[0]
        out.append((np.ascontiguousarray(words).view(np.uint8).copy(),
                    set(zip(esc.tolist(), r[esc].tolist()))))
        beg += c
    return out


def fold_return_buffer(allowed, remaining, seg_counts, w, cap, fill=0):
    """One whole return buffer: fold_return laid out by ret_layout, the first `cap` escapes of
    a segment listed in position order (one of the orders a device may produce)."""
    seg, blk, tot = ret_layout(seg_counts, w, cap)
    buf = np.full(tot, fill, np.uint8)
    for s, (data, esc) in enumerate(fold_return(allowed, remaining, seg_counts, w)):
        buf[seg[s]:seg[s] + data.size] = data
        b = buf[blk[s]:blk[s] + 8 + 16 * cap].view(np.int64)
        b[0] = len(esc)
        for k, (pos, rem) in enumerate(sorted(esc)[:cap]):
            b[1 + 2 * k], b[2 + 2 * k] = pos, rem
    return buf


def unpack_return(buf, seg_counts, w, cap, perm=None):
    """(allowed, remaining, lost) from a return buffer, reading whatever entries its blocks
    hold: an escaped result comes back as (0, its listed remaining), or (0, REMAINING_ERROR)
    and one more in `lost` when the first min(count, cap) entries do not list it."""
    buf = np.asarray(buf, np.uint8)
    seg, blk, _ = ret_layout(seg_counts, w, cap)
    n = int(sum(int(c) for c in seg_counts))
    a_out, r_out, lost, beg = np.zeros(n, np.uint8), np.zeros(n, np.int64), 0, 0
    for s, c in enumerate(seg_counts):
        c = int(c)
        words = buf[seg[s]:seg[s] + c * w].view(_U[w]).astype(np.uint64)
        a, r = unfold_packed(buf[seg[s]:seg[s] + c * w], w)
        esc = np.nonzero(words == ESCAPE)[0]
        if esc.size:
            b = buf[blk[s]:blk[s] + 8 + 16 * cap].view(np.int64)
            cnt = int(min(int(b[0:1].view(np.uint64)[0]), cap))
            found = {}
            for k in range(cnt - 1, -1, -1):                     # the first listing wins
                found[int(b[1 + 2 * k])] = int(b[2 + 2 * k])
            for j in esc.tolist():
                a[j] = 0
                r[j] = found.get(j, REMAINING_ERROR)
                lost += j not in found
        a_out[beg:beg + c], r_out[beg:beg + c] = a, r
        beg += c
    if perm is not None:
        a_out, r_out = scatter(perm, n, a_out, r_out)
    return a_out, r_out, lost


# ---------------------------------------------------------------- compact wire
def pack_wire(perm, keys, permits, now):
    """(wire [n, 2] uint64, base_ms, overflow): wire[j] = {key, (u32)permits << 32 |
    (now_ms - base_ms)} of request perm[j]; base_ms = floorDiv(now[0], 1e6) - 2^31 (0 for an
    empty batch); overflow = 1 when some now_ms lies outside [base_ms, base_ms + 2^32)."""
    perm = np.asarray(perm, np.uint32)
    now = np.asarray(now, np.int64)
    if now.size == 0:
        return np.zeros((0, 2), np.uint64), 0, 0
    base = int(np.floor_divide(now[0], NS)) - 2 ** 31
    rel = np.floor_divide(now[perm], NS) - base
    ovf = int(((rel < 0) | (rel > 0xFFFFFFFF)).any())
    w1 = (np.asarray(permits, np.int32)[perm].view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        (rel.astype(np.uint64) & np.uint64(0xFFFFFFFF))
    return np.stack([np.asarray(keys, np.uint64)[perm], w1], 1), base, ovf


def unwire(wire, bases, counts):
    """(keys, permits, now_ns) of m wire records from len(bases) sources in source order."""
    wire = np.asarray(wire, np.uint64).reshape(-1, 2)
    w1 = wire[:, 1]
    permits = (w1 >> np.uint64(32)).astype(np.uint32).view(np.int32)
    rel = (w1 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    base = np.repeat(np.asarray(bases, np.int64), np.asarray(counts, np.int64))
    return wire[:, 0].copy(), permits, (base + rel) * NS


# ---------------------------------------------------------------- ops column and the wait unpack
def fold_ops(perm, limiter, op):
    """col[j] = min(limiter[perm[j]], 0x3FFF) | min(op[perm[j]], 3) << 14 (either None: 0)."""
    perm = np.asarray(perm, np.uint32)
    l = np.zeros(perm.size, np.uint32) if limiter is None else np.asarray(limiter, np.uint16)[perm].astype(np.uint32)
    o = np.zeros(perm.size, np.uint32) if op is None else np.asarray(op, np.uint8)[perm].astype(np.uint32)
    return (np.minimum(l, 0x3FFF) | (np.minimum(o, 3) << 14)).astype(np.uint16)


def unfold_ops(col):
    col = np.asarray(col, np.uint16)
    return col & np.uint16(0x3FFF), (col >> 14).astype(np.uint8)


def unpack_wait(n, perm, back, n_live):
    """wait[perm[j]] = back[j] for j < n_live; every other request (the skipped ones) 0."""
    wait = np.zeros(n, np.int64)
    wait[np.asarray(perm, np.uint32)[:n_live]] = np.asarray(back, np.int64)[:n_live]
    return wait
