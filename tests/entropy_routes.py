"""The stage after the BBWT gather - move-to-front (csrc/k_mtf.hip), the five Rice sizes it
accumulates, the xor / lfsr counters, k_mdl and payload emission (csrc/k_entropy.hip) - as a plain
numpy model, a route predictor and a route matrix of named cases, for
tests/test_entropy_route_model.py and tests/test_gpu_entropy_routes.py ("route matrix
of the MTF, size, MDL and emission stage").

Inputs.  BBWT is a bijection and every byte sequence is a valid MTF index sequence, so a row chooses
the MTF indices m it wants the device to produce and derives the block:
block = bbwt_inverse(mtf_decode(m)).  The device's BBWT -> MTF of that block must give m back, and
every expectation follows from m alone (no CPU BBWT): the sizes of methods 2..6 are the Rice bit
lengths of m under the five maps, the payloads their Rice codes.  The rows about geometry choose the
BBWT output L instead (skewed random bytes), m = mtf(L).  The xor / lfsr row chooses the block's own
bytes; its m comes from the oracle's BBWT and MTF.

Model.  maps / rice_bits / rice_code / uleb / mdl below restate the formats, not the kernels: one
symbol at a time in numpy, no tiles, no words.

Predictor.  predict() restates the selection conditions of the code from the geometry, the index
values and the payload offsets alone, and names every route the batch takes (ROUTES).  The per-thread
paths leave no trace on the device; that a row reaches them is shown by the predictor on the CPU."""
import functools

import numpy as np

import oracle as O
from kolm import decode as H

NCAND = 11
OFF = 0xFFFFFFFF             # size of a disabled candidate
RICE_IDS = (2, 3, 4, 5, 6)   # plain, bit-plane, nibble swap, bit reverse, Gray
FLAG_OF = {2: 0, 3: 1, 4: 4, 5: 8, 6: 16}
RICE_K = 2                   # the batched path's Rice parameter
NO_LZ = 0x17F                # ids 0..6 and 8: every size of it comes from the model
TILE = 2048                  # symbols per emission tile: 256 threads of 8
CHEAP_T = 4096               # bytes per workgroup of k_cheap_sizes (16 per thread)
CP_R = 128                   # compose ranges per block
MTF_CHUNK = 1024


# ------------------------------------------------------------------ model: maps, Rice, ULEB, MDL

_BITREV = np.array([int(f"{i:08b}"[::-1], 2) for i in range(256)], dtype=np.uint8)


def bitplane(m):
    """8-byte groups, the last zero padded: plane b's value has byte i's bit (7 - b) at bit 7 - i."""
    m = np.asarray(m, np.uint8)
    g = np.zeros((len(m) + 7) // 8 * 8, np.uint8)
    g[:len(m)] = m
    bits = np.unpackbits(g.reshape(-1, 8), axis=1).reshape(-1, 8, 8)  # [group][byte i][column b] = bit 7 - b of byte i
    return np.packbits(bits.transpose(0, 2, 1).reshape(-1, 8), axis=1).ravel()


def mapped(m, mid):
    """The symbols method `mid` (2..6) codes for the MTF indices m."""
    m = np.asarray(m, np.uint8)
    if mid == 2:
        return m
    if mid == 3:
        return bitplane(m)
    if mid == 4:
        return ((m & 0x0F) << 4) | (m >> 4)
    if mid == 5:
        return _BITREV[m]
    if mid == 6:
        return m ^ (m >> 1)
    raise ValueError(mid)


def rice_bits(v, k):
    """Bit length of every symbol's Rice code: (v >> k) + 1 + k."""
    return (np.asarray(v, np.int64) >> k) + 1 + k


def rice_code(v, k):
    """Rice code of the symbols, MSB first: v >> k ones, a zero, then the low k bits."""
    v = np.asarray(v, np.int64)
    if not len(v):
        return b""
    ln = rice_bits(v, k)
    start = np.cumsum(ln) - ln
    q = v >> k
    d = np.zeros(int(ln.sum()) + 1, np.int32)
    np.add.at(d, start, 1)
    np.add.at(d, start + q, -1)
    bits = np.cumsum(d[:-1]).astype(np.uint8)  # the unary runs
    for j in range(k):
        bits[start + q + 1 + j] = (v >> (k - 1 - j)) & 1
    return np.packbits(bits).tobytes()


@functools.lru_cache(maxsize=None)
def lfsr_table():
    """s_i = LFSR^i(1), taps 0x96: period 255."""
    t, s = [], 1
    for _ in range(255):
        t.append(s)
        fb = bin(s & 0x96).count("1") & 1
        s = ((s << 1) & 0xFF) | fb
    assert s == 1 and len(set(t)) == 255
    return np.array(t, np.uint8)


def deltas(block, mid):
    """The byte deltas of xor (1: against the previous byte, 0 before the first) and lfsr (8:
    against the LFSR sequence, whose phase restarts at the block's first byte)."""
    t = np.frombuffer(block, np.uint8)
    if mid == 1:
        ref = np.concatenate([[0], t[:-1]]).astype(np.uint8)
    else:
        ref = lfsr_table()[np.arange(len(t)) % 255]
    return t - ref  # uint8 arithmetic wraps


def uleb(d):
    """ULEB128 of byte values: one byte under 128, else the low 7 bits with the top bit set, then 1."""
    d = np.asarray(d, np.uint8)
    big = d >= 128
    out = np.zeros(len(d) + int(big.sum()), np.uint8)
    at = np.arange(len(d)) + np.cumsum(big) - big
    out[at] = np.where(big, (d & 0x7F) | 0x80, d)
    out[at[big] + 1] = d[big] >> 7
    return out.tobytes()


def block_sizes(block, m):
    """Sizes of candidates 0..6 and 8 of a block with MTF indices m (7, 9, 10: None)."""
    n = len(block)
    sz = [None] * NCAND
    sz[0] = n
    sz[1] = n + int((deltas(block, 1) >= 128).sum())
    for mid in RICE_IDS:
        sz[mid] = (int(rice_bits(mapped(m, mid), RICE_K).sum()) + 7) // 8
    sz[8] = n + int((deltas(block, 8) >= 128).sum())
    return sz


def payload(block, m, mid, k=RICE_K):
    """Payload of candidates 0..6 and 8 from the model; 7 (LZ77) is the oracle's."""
    if mid == 0:
        return bytes(block)
    if mid in (1, 8):
        return uleb(deltas(block, mid))
    if mid in RICE_IDS:
        return rice_code(mapped(m, mid), k)
    if mid == 7:
        return O.candidate(7, block)
    raise ValueError(mid)


def mdl(sizes, mask, force=-1):
    """(sizes as the device reports them, winner): a disabled id reads 0xFFFFFFFF; the winner is the
    enabled id with the strictly smallest size, so ties go to the lowest id; nothing enabled -> raw;
    force >= 0 overrides."""
    rep = [int(s) if (mask >> i) & 1 and s is not None else OFF for i, s in enumerate(sizes)]
    best, bsz = 0, None
    for i, s in enumerate(sizes):
        if (mask >> i) & 1 and s is not None and (bsz is None or s < bsz):
            best, bsz = i, s
    return rep, (int(force) if force >= 0 else best)


# ------------------------------------------------------------------ blocks from chosen indices

class Blk:
    """One block: its bytes, its BBWT L and its MTF indices m.  chosen: m (or L) was chosen and the
    block derived through the host decoder; otherwise the bytes were chosen and L, m are the oracle's."""

    def __init__(self, block, L, m, chosen=True):
        self.block, self.L, self.m, self.chosen = bytes(block), bytes(L), np.frombuffer(bytes(m), np.uint8), chosen
        self.n = len(self.block)


@functools.lru_cache(maxsize=None)
def _from_m(m):
    L = H.mtf_decode(m)
    return Blk(H.bbwt_inverse(L), L, m)


def from_m(m):
    return _from_m(bytes(np.asarray(m, np.uint8)))


@functools.lru_cache(maxsize=None)
def from_L(L):
    return Blk(H.bbwt_inverse(L), L, O.mtf_encode(L))


@functools.lru_cache(maxsize=None)
def from_bytes(block):
    L = O.bbwt_forward(block)
    return Blk(block, L, O.mtf_encode(L), chosen=False)


def _rng(seed):
    return np.random.default_rng(seed)


def geometric(seed, n, p=0.35):
    """Indices with a geometric law: mostly 0..7 (the replay's register entries), a tail into the LDS."""
    return np.minimum(_rng(seed).geometric(p, n) - 1, 255).astype(np.uint8)


def skewed_L(seed, n):
    """BBWT-like output for the geometry rows: runs of a few symbols from a skewed alphabet."""
    r = _rng(seed)
    sym = np.minimum(r.geometric(0.08, n) - 1, 255).astype(np.uint8)
    keep = r.random(n) < 0.6  # 60 %: repeat the previous symbol
    idx = np.maximum.accumulate(np.where(keep, 0, np.arange(n)))
    return (sym[idx] * 37 + 11).astype(np.uint8).tobytes()


# ------------------------------------------------------------------ the route predictor

ROUTES = (
    # which replay kernel, and the threshold between them
    "mtf.wave", "mtf.replay", "mtf.wave.nb63", "mtf.replay.nb64",
    # bytes per chunk (mtf_chunk_bytes)
    "wave.csz1024", "replay.csz128", "replay.csz256", "replay.csz512", "replay.csz1024",
    # k_mtf_summary
    "summary.wholewg", "summary.16", "summary.byte", "summary.past_end", "summary.count256",
    # k_mtf_replay: the three access paths (RiceAcc add4 / add4 / add), list entries in registers / LDS
    "replay.64", "replay.16", "replay.byte", "replay.16_and_byte",
    "acc.add4", "acc.add", "acc.lane",
    "replay.reg0", "replay.reg1", "replay.lds", "replay.lds_every_chunk", "replay.w63_j3", "replay.w63_j012",
    # k_mtf_wave
    "wave.partial_step", "wave.short_group", "wave.unaligned_base",
    # the bit-plane group of a block's last bytes, zero padded
    "bp.pad",
    # k_mtf_cp1..3
    "cp.empty_range", "cp.multi_chunk_range", "cp.one_byte_block",
    # k_rice_emit
    "emit.fast", "emit.fast_3words", "emit.slow", "emit.q32_loop", "emit.split_unary", "emit.put_split",
    "emit.len64", "emit.len66", "emit.ns_lt8", "emit.one_word_tile", "emit.tile_leads_all32",
    "emit.blockstart.lead0", "emit.blockstart.lead8", "emit.blockstart.lead16", "emit.blockstart.lead24",
    "emit.edge_prev.raw", "emit.edge_prev.xor", "emit.edge_prev.lfsr", "emit.edge_prev.lz77", "emit.edge_prev.rice",
    "emit.edge_next.raw", "emit.edge_next.xor", "emit.edge_next.lfsr", "emit.edge_next.lz77", "emit.edge_next.rice",
    # k_mdl
    "mdl.win2", "mdl.win3", "mdl.win4", "mdl.win5", "mdl.win6", "mdl.tie_lowest", "mdl.mask0_refused", "mdl.force",
    # k_cheap_sizes, k_simple_count, k_emit_simple
    "cheap.aligned", "cheap.unaligned", "cheap.tail", "simple.odd_base", "simple.uleb2_tile_edge.xor",
    "simple.uleb2_tile_edge.lfsr", "simple.lfsr_wrap",
)
_KIND = {0: "raw", 1: "xor", 8: "lfsr", 7: "lz77", 2: "rice", 3: "rice", 4: "rice", 5: "rice", 6: "rice"}


def is_fixed(lens):
    """The batch goes through the fixed-geometry entry: equal blocks, the last one not longer."""
    return all(x == lens[0] for x in lens[:-1]) and lens[-1] <= lens[0]


def wave_mode(nb, switch=None):
    """mtf_wave_mode: KOLM_MTF_WAVE = 0 / 1 forces; otherwise batches under 64 blocks."""
    return bool(switch) if switch is not None else nb < 64


def chunk_bytes(bs, nb, wave):
    """mtf_chunk_bytes: 1 KiB in the wave form; else halved while ceil(bs / csz) * nb < 16384, down to 128."""
    csz = MTF_CHUNK
    if wave:
        return csz
    while csz > 128 and -(-bs // csz) * nb < 16384:
        csz >>= 1
    return csz


class Prediction:
    """routes: the names of ROUTES the batch takes.  kernel / csz / cpb / summary_bytes: the device
    evidence (the replay kernel launched; the bytes launch_mtf records for k_mtf_summary)."""


def predict(blks, methods, paylens, mask_used=None, switch=None, ties=None, forced=False):
    """blks: the batch's Blk; methods: every block's winner; paylens: every block's payload size;
    switch: KOLM_MTF_WAVE (None unset, 0, 1).  What k_mdl was asked: mask_used, forced, and per block
    ties (the smallest enabled size is shared by two ids or more)."""
    lens = np.array([b.n for b in blks], np.int64)
    nb, N = len(lens), int(lens.sum())
    fixed = is_fixed(lens.tolist())
    bs = int(lens[0]) if fixed else int(lens.max())
    base = (np.arange(nb) * bs) if fixed else np.concatenate([[0], np.cumsum(lens)[:-1]])
    end = base + lens
    m = np.concatenate([b.m for b in blks])
    L = np.frombuffer(b"".join(b.L for b in blks), np.uint8)
    text = np.frombuffer(b"".join(b.block for b in blks), np.uint8)
    R = set()
    P = Prediction()

    # ---- MTF
    wave = wave_mode(nb, switch)
    csz = chunk_bytes(bs, nb, wave)
    cpb = -(-bs // csz)
    P.kernel, P.csz, P.cpb, P.summary_bytes = ("k_mtf_wave" if wave else "k_mtf_replay"), csz, cpb, N + 256 * cpb * nb
    R.add("mtf.wave" if wave else "mtf.replay")
    if switch is None and nb == 63:
        R.add("mtf.wave.nb63")
    if switch is None and nb == 64:
        R.add("mtf.replay.nb64")
    R.add("wave.csz1024" if wave else f"replay.csz{csz}")
    c = np.arange(cpb * nb)
    cb, ck = c // cpb, c % cpb
    lo = base[cb] + ck * csz
    hi = np.minimum(lo + csz, end[cb])
    valid = lo < end[cb]
    # k_mtf_summary: a launch group of 256 chunks takes the whole-workgroup path when every one of
    # them is a full chunk at a 16-byte boundary
    full = valid & (hi - lo == csz) & ((lo & 15) == 0)
    pad = np.zeros(-(-len(c) // 256) * 256, bool)
    pad[:len(c)] = full
    whole = np.repeat(pad.reshape(-1, 256).all(axis=1), 256)[:len(c)]
    a16 = ((lo | hi) & 15) == 0
    for name, sel in (("summary.wholewg", whole), ("summary.16", valid & ~whole & a16),
                      ("summary.byte", valid & ~whole & ~a16), ("summary.past_end", ~valid)):
        if sel.any():
            R.add(name)
    for i in np.flatnonzero(valid & (hi - lo >= 256)):
        if len(np.unique(L[lo[i]:hi[i]])) == 256:
            R.add("summary.count256")
            break
    vlo = lo[valid]
    assert (np.sort(vlo) == vlo).all() and vlo[0] == 0  # the valid chunks tile the batch in order
    if wave:
        R.add("acc.lane")
        if (((hi - lo) % 64 != 0) & valid).any():
            R.add("wave.partial_step")
        if (((hi - lo) % 8 != 0) & valid).any():
            R.add("wave.short_group")
        if (((lo & 15) != 0) & valid).any():
            R.add("wave.unaligned_base")
    else:
        a64 = ((lo | hi) & 63) == 0
        p64, p16, pb = valid & a64, valid & ~a64 & a16, valid & ~a16
        for name, sel in (("replay.64", p64), ("replay.16", p16), ("replay.byte", pb)):
            if sel.any():
                R.add(name)
        if p16.any() and pb.any():
            R.add("replay.16_and_byte")
        if p64.any() or p16.any():
            R.add("acc.add4")
        if pb.any():
            R.add("acc.add")
        # the recency list: entries 0..3 and 4..7 in two registers, the rest in LDS words 2..63
        for name, sel in (("replay.reg0", m < 4), ("replay.reg1", (m >= 4) & (m < 8)), ("replay.lds", m >= 8),
                          ("replay.w63_j3", m == 255), ("replay.w63_j012", (m >= 252) & (m < 255))):
            if sel.any():
                R.add(name)
        if (np.maximum.reduceat(m, vlo) >= 8).all():
            R.add("replay.lds_every_chunk")
    if (lens % 8 != 0).any():
        R.add("bp.pad")
    # compose: a block's nch chunks in 128 ranges of per = ceil(nch / 128)
    nch = -(-lens // csz)
    per = -(-nch // CP_R)
    if (np.minimum((CP_R - 1) * per, nch) == nch).any():
        R.add("cp.empty_range")  # the last range starts at nch
    if (per > 1).any():
        R.add("cp.multi_chunk_range")
    if (lens == 1).any():
        R.add("cp.one_byte_block")

    # ---- MDL
    methods = [int(x) for x in methods]
    if forced:
        R.add("mdl.force")
    elif mask_used == 0:
        R.add("mdl.mask0_refused")  # the entry points answer KOLM_EARG: k_mdl's raw fall-back is the model's alone
    else:
        for b, w in enumerate(methods):
            if ties is not None and ties[b]:
                R.add("mdl.tie_lowest")
            elif w in RICE_IDS:
                R.add(f"mdl.win{w}")  # the unique minimum

    # ---- emission
    off = np.concatenate([[0], np.cumsum(paylens)]).astype(np.int64)
    leads = set()
    for b, mid in enumerate(methods):
        if mid in RICE_IDS:
            _predict_rice(R, leads, mapped(blks[b].m, mid), int(blks[b].n), int(off[b]))
            R.add(f"emit.blockstart.lead{(off[b] * 8) % 32}")
            if off[b] % 4 and b:
                R.add("emit.edge_prev." + _KIND[methods[b - 1]])
            if off[b + 1] % 4 and b + 1 < nb:
                R.add("emit.edge_next." + _KIND[methods[b + 1]])
    if len(leads) == 32:
        R.add("emit.tile_leads_all32")

    # ---- xor / lfsr sizes (every block) and their emission (blocks that chose them)
    for b in range(nb):
        g0 = np.arange(base[b], end[b], 16)
        tail = (end[b] - g0) < 16
        if (~tail & ((g0 & 15) == 0)).any():
            R.add("cheap.aligned")
        if (~tail & ((g0 & 15) != 0)).any():
            R.add("cheap.unaligned")
        if tail.any():
            R.add("cheap.tail")
        if methods[b] in (1, 8):
            if base[b] & 1:
                R.add("simple.odd_base")
            big = deltas(blks[b].block, methods[b]) >= 128
            edges = np.arange(TILE, lens[b], TILE)
            if len(edges) >= 2 and (big[edges - 1] & big[edges]).any():
                R.add("simple.uleb2_tile_edge." + _KIND[methods[b]])
            if methods[b] == 8:
                wrap = np.arange(254, lens[b] - 1, 255)
                if (big[wrap] & big[wrap + 1]).any():
                    R.add("simple.lfsr_wrap")
    assert text.size == N
    P.routes = R
    return P


def _predict_rice(R, leads, sym, n, off_bytes, k=RICE_K):
    """k_rice_emit on one block's symbols: a thread codes the 8 symbols of an 8-byte group of the
    index sequence (all 8 plane values for the bit-plane map, the valid ones otherwise); a tile is
    256 threads; `lead` is the tile's first bit modulo 32."""
    ln = rice_bits(sym, k)
    nthr = -(-n // 8)
    ns = np.full(nthr, 8)
    if len(sym) < nthr * 8:
        ns[-1] = len(sym) - (nthr - 1) * 8
    lp = np.zeros(nthr * 8, np.int64)
    lp[:len(ln)] = ln
    cnt = lp.reshape(-1, 8).sum(axis=1)
    start = off_bytes * 8 + np.cumsum(cnt) - cnt  # every thread's first bit in the arena
    o = start % 32
    fast = cnt <= 64
    if fast.any():
        R.add("emit.fast")
    if (fast & (o + cnt > 64)).any():
        R.add("emit.fast_3words")
    if (ns < 8).any():
        R.add("emit.ns_lt8")
    thr = np.repeat(np.arange(nthr), 8)[:len(sym)]
    if (fast[thr] & (ln >= 64)).any():
        R.add("emit.len64")
    if (ln == 66).any():
        R.add("emit.len66")
    slow = ~fast[thr]
    if slow.any():
        R.add("emit.slow")
        q = (np.asarray(sym, np.int64) >> k)[slow]
        so = ((off_bytes * 8 + np.cumsum(ln) - ln) % 32)[slow]  # the symbol's first bit modulo 32
        if (q >= 32).any():
            R.add("emit.q32_loop")
        qr = q % 32
        two = qr + 1 + k > 32
        if two.any():
            R.add("emit.split_unary")
        split = ((q >= 32) & (so != 0)) | (~two & (so + qr + 1 + k > 32)) | (two & (so + qr > 32)) \
            | (two & ((so + qr) % 32 + 1 + k > 32))
        if split.any():
            R.add("emit.put_split")
    for t0 in range(0, nthr, TILE // 8):
        tot = int(cnt[t0:t0 + TILE // 8].sum())
        lead = int(start[t0] % 32)
        leads.add(lead)
        if (lead + tot + 31) >> 5 == 1:
            R.add("emit.one_word_tile")


# ------------------------------------------------------------------ the route matrix

class Run:
    """One encode call of a case: the candidate mask, and the forced method of every block (None:
    nothing forced)."""

    def __init__(self, mask, force=None):
        self.mask, self.force = mask, force


class Case:
    """One row: make() -> the batch's Blk; runs: its encode calls; claims: the routes the row is
    there for (test_entropy_route_model requires predict() to name each of them); mtf: the row runs
    again with KOLM_MTF_WAVE set to the opposite form; opposite: routes the row claims in that form."""

    def __init__(self, name, make, claims, runs=None, mtf=False, opposite=()):
        self.name, self.make, self.claims, self.mtf, self.opposite = name, make, tuple(claims), mtf, tuple(opposite)
        self._runs = runs

    @functools.lru_cache(maxsize=None)
    def blks(self):
        return tuple(self.make())

    def blocks(self):
        return [b.block for b in self.blks()]

    def runs(self):
        return self._runs(self.blks()) if self._runs else [Run(NO_LZ)]

    def model(self, run):
        """(sizes as reported [nb][11], winners, payloads) of one run."""
        sizes, win, pays = [], [], []
        for i, b in enumerate(self.blks()):
            f = -1 if run.force is None else int(run.force[i])
            rep, w = mdl(_sizes(b), run.mask, f)
            sizes.append(rep)
            win.append(w)
            pays.append(_payload(b, w))
        return np.array(sizes, np.uint32), win, pays

    def predict(self, run, switch=None):
        _, win, pays = self.model(run)
        ties = None
        if run.force is None and run.mask:
            ties = []
            for b in self.blks():
                en = [s for i, s in enumerate(_sizes(b)) if (run.mask >> i) & 1 and s is not None]
                ties.append(en.count(min(en)) > 1)
        return predict(self.blks(), win, [len(p) for p in pays], mask_used=run.mask, switch=switch, ties=ties,
                       forced=run.force is not None)


@functools.lru_cache(maxsize=None)
def _sizes_cached(blk):
    return tuple(block_sizes(blk.block, blk.m))


def _sizes(blk):
    return list(_sizes_cached(blk))


@functools.lru_cache(maxsize=None)
def _payload(blk, mid):
    return payload(blk.block, blk.m, mid)


def _force_all(mid, mask=NO_LZ):
    return lambda blks: [Run(mask, [mid] * len(blks))]


# -- MTF rows

@functools.lru_cache(maxsize=None)
def _thousand():
    return [from_m(geometric(100 + i, 1000, 0.2 + 0.01 * (i % 30))) for i in range(64)]


@functools.lru_cache(maxsize=None)
def _big_L():
    """128 KiB of skewed BBWT output; bytes 2048..2303 hold all 256 symbols (one chunk of 256 bytes or
    more then has a summary of 256 entries)."""
    L = bytearray(skewed_L(7, 1 << 17))
    L[2048:2304] = bytes(_rng(8).permutation(256).astype(np.uint8))
    return bytes(L)


@functools.lru_cache(maxsize=None)
def _eight_32k():
    return [skewed_L(20 + i, 1 << 15) for i in range(8)]


def _wholewg():
    return [from_L(_eight_32k()[i % 8]) for i in range(64)]


def _ragged():
    """Block bounds: 30 blocks of 32 KiB, one 48 bytes shorter (every later block then starts 16 past
    a multiple of 64), 32 of 32 KiB, and a last one of 32 KiB - 1005 bytes."""
    n = 1 << 15
    lens = [n] * 30 + [n - 48] + [n] * 32 + [n - 1005]
    return [from_L(_eight_32k()[i % 8][:ln]) for i, ln in enumerate(lens)]


def _odd_lens():
    """127 odd lengths from 1 to 1499, some of them 1."""
    return [1 if i % 16 == 0 else 1 + 2 * ((i * 37) % 750) for i in range(127)]


@functools.lru_cache(maxsize=None)
def _odd_blocks():
    return [from_m(geometric(300 + i, ln, 0.25)) for i, ln in enumerate(_odd_lens())]


def _replay_var(first):
    return lambda: [from_L(_big_L()[:first])] + _odd_blocks()


def _deep():
    """Three blocks.  0: uniform indices, and in every 128 bytes the explicit 255, 252, 253, 254 (the
    last LDS word, byte 3 and bytes 0..2).  1: only indices 8..255.  2: index 255 throughout, so L
    walks through all 256 symbols in every 256 bytes."""
    r = _rng(41)
    a = r.integers(0, 256, 8192, dtype=np.uint8)
    a.reshape(-1, 128)[:, 5:9] = [255, 252, 253, 254]
    b = r.integers(8, 256, 8192 - 40, dtype=np.uint8)
    c = np.full(2048 + 24, 255, np.uint8)
    return [from_m(a), from_m(b), from_m(c)]


def _odd_base():
    """Block bounds under 64 blocks: the bases are 4097, 6151, 7183 = 1, 7, 15 modulo 16."""
    return [from_m(geometric(50 + i, ln)) for i, ln in enumerate((4097, 2054, 1032, 3000))]


# -- emission and MDL rows

def _slow():
    """Per-thread codes over 64 bits: a 16 KiB block of index 255 (66 bits a symbol: the largest
    payload there is), a block of index 200, and one of mixed indices 128..255."""
    return [from_m(np.full(1 << 14, 255, np.uint8)), from_m(np.full(4096, 200, np.uint8)),
            from_m(_rng(61).integers(128, 256, 4096 + 3, dtype=np.uint8))]


def _edge64():
    """Tails of 1..7 symbols; in the first block the last thread holds one symbol whose code is
    exactly 64 bits (index 245: 61 ones, a zero, two bits)."""
    out = []
    for t in range(1, 8):
        m = geometric(70 + t, 800 + t)
        if t == 1:
            m[-1] = 245
        out.append(from_m(m))
    return out


def _winner_each():
    return [from_m(np.full(4096, c, np.uint8)) for c in (0x08, 0x99, 0x10, 0x40, 0x0C)]


def _ties():
    return [from_m(np.zeros(n, np.uint8)) for n in (64, 8, 4096)]


def _tie_runs(blks):
    """Every non-empty subset of ids 2..6, and the empty mask (which the entry points refuse with
    KOLM_EARG before any kernel runs: the rule "nothing enabled -> raw" is checked on the model alone)."""
    return [Run(s << 2) for s in range(1, 32)] + [Run(0)]


MOSAIC_ORDER = (2, 0, 3, 1, 4, 8, 5, 7, 6)


def _mosaic():
    """36 adjacent blocks of mixed lengths; two of them one byte over a tile (a one-byte last tile)."""
    r = _rng(81)
    lens = [int(x) for x in r.integers(40, 700, 36)]
    lens[0] = lens[9] = TILE + 1
    return [from_m(geometric(400 + i, ln, 0.3)) for i, ln in enumerate(lens)]


def _mosaic_runs(blks):
    return [Run(NO_LZ, [MOSAIC_ORDER[i % 9] for i in range(len(blks))])]


def _simple():
    """xor / lfsr on blocks longer than two tiles at odd bases.  The bytes are chosen: at both sides of
    the first tile edge (2047, 2048) the delta is 200, and for lfsr also at phases 254 and 0 (254, 255)."""
    lf = lfsr_table()
    out = [from_bytes(b"\x07")]
    for i, (mid, n) in enumerate(((1, 5000), (8, 4611), (1, 4100), (8, 4099))):
        t = _rng(90 + i).integers(0, 256, n, dtype=np.uint8)
        for p in (2047, 2048) + ((254, 255) if mid == 8 else ()):
            t[p] = (int(t[p - 1]) + 200) & 0xFF if mid == 1 else (int(lf[p % 255]) + 200) & 0xFF
        out.append(from_bytes(t.tobytes()))
    return out


def _simple_runs(blks):
    return [Run(NO_LZ, [0, 1, 8, 1, 8])]


def _cases():
    c = []

    def add(*a, **k):
        c.append(Case(*a, **k))
    add("wave_one_block", lambda: [from_m(geometric(1, 4096 + 256 + 63))],
        ("mtf.wave", "wave.csz1024", "wave.partial_step", "wave.short_group", "acc.lane", "bp.pad"), mtf=True)
    add("wave_63_blocks", lambda: _thousand()[:63], ("mtf.wave", "mtf.wave.nb63", "summary.byte"), mtf=True)
    add("replay_64_blocks", lambda: _thousand()[:64],
        ("mtf.replay", "mtf.replay.nb64", "replay.csz128", "replay.byte", "acc.add", "summary.byte",
         "replay.reg0", "replay.reg1", "replay.lds"), mtf=True)
    add("replay_128_wholewg", _wholewg,
        ("mtf.replay", "replay.csz128", "summary.wholewg", "replay.64", "acc.add4", "cp.multi_chunk_range",
         "emit.tile_leads_all32", "emit.fast", "emit.fast_3words"), mtf=True)
    add("replay_128_ragged", _ragged,
        ("mtf.replay", "replay.csz128", "summary.wholewg", "summary.16", "summary.byte", "summary.past_end",
         "replay.64", "replay.16", "replay.byte", "replay.16_and_byte", "bp.pad"), mtf=True)
    for first, csz in ((1 << 15, 256), (1 << 16, 512), (1 << 17, 1024)):
        add(f"replay_{csz}", _replay_var(first),
            ("mtf.replay", f"replay.csz{csz}", "replay.byte", "summary.byte", "summary.count256", "cp.empty_range",
             "cp.one_byte_block", "summary.past_end"), mtf=True)
    add("deep_indices", _deep, ("mtf.wave", "summary.count256"), mtf=True,
        # (raw wins these blocks: a second run forces method 2, so that their Rice payloads are compared too)
        runs=lambda blks: [Run(NO_LZ), Run(NO_LZ, [2] * len(blks))],
        opposite=("mtf.replay", "replay.csz128", "replay.lds", "replay.lds_every_chunk", "replay.w63_j3",
                  "replay.w63_j012"))
    add("odd_base_var", _odd_base, ("mtf.wave", "wave.unaligned_base", "wave.partial_step", "cheap.unaligned"), mtf=True)
    add("rice_slow_k2", _slow, ("emit.slow", "emit.q32_loop", "emit.split_unary", "emit.put_split", "emit.len66",
                                "mdl.force"), _force_all(2))
    add("rice_edge_64", _edge64, ("emit.len64", "emit.ns_lt8", "emit.fast", "mdl.force"), _force_all(2))
    add("winner_each", _winner_each, ("mdl.win2", "mdl.win3", "mdl.win4", "mdl.win5", "mdl.win6"),
        lambda blks: [Run(0x7C)])
    add("ties", _ties, ("mdl.tie_lowest", "mdl.mask0_refused"), _tie_runs)
    add("mosaic", _mosaic,
        ("mdl.force", "emit.one_word_tile", "emit.blockstart.lead0", "emit.blockstart.lead8", "emit.blockstart.lead16",
         "emit.blockstart.lead24") + tuple(f"emit.edge_{d}.{k}" for d in ("prev", "next")
                                           for k in ("raw", "xor", "lfsr", "lz77", "rice")), _mosaic_runs)
    add("simple_tiles", _simple,
        ("mdl.force", "simple.odd_base", "simple.uleb2_tile_edge.xor", "simple.uleb2_tile_edge.lfsr", "simple.lfsr_wrap",
         "cheap.unaligned", "cheap.aligned", "cheap.tail"), _simple_runs)
    return {x.name: x for x in c}


CASES = _cases()
MTF_ROWS = tuple(n for n, x in CASES.items() if x.mtf)


def opposite_switch(case):
    """KOLM_MTF_WAVE for the form the row does not take by default."""
    return 0 if wave_mode(len(case.blks())) else 1


def predicted_routes(case, switch=None):
    """The union of predict() over the case's runs (for `ties`: over its masks)."""
    out = set()
    for run in case.runs():
        out |= case.predict(run, switch).routes
    return out
