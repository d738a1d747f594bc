"""Inputs that steer the omega-order sort's doubling rounds (csrc/k_sort.hip, sort_pass in
csrc/kolm_api.cpp) onto chosen routes, and a plain numpy model of those rounds, for
tests/test_sort_route_model.py and tests/test_gpu_sort_routes.py ("route matrix").

Builder.  A block is b"\\x00" (the unique minimum: the block is one Lyndon word, all its rotations
are distinct) followed by families and optional random filler.  A family (G, L) is G copies of a
random word W of L bytes (values 1..255), each copy followed by a 3-byte separator (values 1..255)
that is unique in the block.  For every offset j of W the G copies tie until the compared prefix
passes the end of W, so a family gives about L groups of exactly G elements in doubling round 1
and fewer in each later round, up to h ~ L.  Everything is seeded.

Model.  Prefix doubling over the cyclic successor inside each Lyndon factor (factor starts from
the oracle's Duval): the groups of doubling round r >= 1 are the classes of positions whose
rotations agree on 8 * 2^(r-1) characters, with at least two members.  A block is retired after
the first round that changes none of its groups.  That is what the device does when round 0 holds
exactly 8 whole characters: KOLM_R0_CODE=0 and a batch whose widest block has 129..256 distinct
bytes (8-bit fixed codes).  With prefix-code keys round 0 holds 8 or more characters, the device's
groups are refinements of the model's, and its active counts can only be lower."""
import functools

import numpy as np

import oracle as O

TILE = 2048    # largest segment of the one-workgroup LDS sorts (classes 1..11)
MED_T = 8192   # largest segment of the medium sort
NCLASS = 12    # size classes 0..11; index NCLASS of a histogram = "large" (> TILE)
H0 = 8         # characters of round 0 in the fixed 8-bit form


def size_class(n):
    """Class of a segment of n elements: 0 for 1, k for 2^(k-1) < n <= 2^k."""
    return 0 if n <= 1 else int(n - 1).bit_length()


def bitlen(v):
    return int(v).bit_length()


def msd_levels(bs):
    """MSD levels of a doubling round: 8-bit digits of the bitlen(bs)-bit rank keys, the last narrower."""
    return (max(bitlen(bs), 1) + 7) // 8


# ------------------------------------------------------------------ builder

class Fam:
    """G copies of one random word of L bytes.  two: bytes 8..15 of the copies alternate between
    two fixed values (a group of G splits into two equal-key buckets of G/2).  pin: bytes 8.. of
    the word are 0xFF, so the successor ranks the copies are sorted by are the block's highest."""

    def __init__(self, G, L, two=False, pin=False):
        assert G >= 1 and L >= 1 and (not two or L >= 16)
        self.G, self.L, self.two, self.pin = G, L, two, pin


def _rand(rng, n, lo=1):
    return rng.integers(lo, 256, n, dtype=np.uint8)


def build_block(seed, fams, filler=0, lead=True, length=None, split=False):
    """lead=False drops the leading zero: a block of several Lyndon factors.  length: the filler
    is sized so that the block has exactly that many bytes.  split (with lead=False): every
    family, and the filler, is a Lyndon factor of its own - it starts with a byte smaller than
    all of its other bytes, and these first bytes decrease from family to family; the block then
    ends in three one-byte factors b"\\x01" (factors shorter than any h: rotations that wrap
    several times inside a key)."""
    rng = np.random.default_rng(seed)
    fams = [f if isinstance(f, Fam) else Fam(*f) for f in fams]
    assert not (split and lead)
    nchunk = len(fams) + (1 if filler or length is not None else 0)
    lo = nchunk + 1 if split else 1  # the values of words, separators and filler: lo..255
    nv = 256 - lo
    ncopy = sum(f.G for f in fams)
    seps = rng.choice(nv ** 3, ncopy, replace=False)  # distinct 3-digit numbers in base nv
    sep3 = np.stack([seps // (nv * nv), seps // nv % nv, seps % nv], axis=1).astype(np.uint8) + lo
    parts = [np.zeros(1, np.uint8)] if lead else []
    s = 0
    for k, f in enumerate(fams):
        w = _rand(rng, f.L, lo)
        if f.pin:
            w[8:] = 0xFF
        rows = np.tile(w, (f.G, 1))
        if f.two:
            a, b = _rand(rng, 8, lo), _rand(rng, 8, lo)
            rows[0::2, 8:16] = a
            rows[1::2, 8:16] = b
        if split:
            parts.append(np.array([nchunk - k], np.uint8))
        parts.append(np.concatenate([rows, sep3[s:s + f.G]], axis=1).reshape(-1))
        s += f.G
    tail = 3 if split else 0
    body = sum(len(p) for p in parts) + tail + (1 if split and nchunk > len(fams) else 0)
    if length is not None:
        assert length >= body, (length, body)
        filler = length - body
    if filler:
        if split:
            parts.append(np.array([1], np.uint8))
        parts.append(_rand(rng, filler, lo))
    if split:
        parts.append(np.ones(tail, np.uint8))
    return np.concatenate(parts).tobytes()


def periodic_block(seed, L, reps):
    """A word repeated with no separators.  The word is \\x01 followed by L - 1 random bytes of
    2..255, a Lyndon word, so the block's Lyndon factors are its `reps` copies and the rotations
    at the same offset of every copy tie for ever: no doubling round can split them."""
    w = np.random.default_rng(seed).integers(2, 256, L, dtype=np.uint8)
    w[0] = 1
    return bytes(w) * reps


def small_block(seed, n=96):
    """A tiny block that only raises a batch's block count: the 8-byte windows of n random bytes
    are distinct, so round 0 resolves it (the model confirms that for every batch it is used in)."""
    return build_block(seed, [], filler=n - 1)



# ------------------------------------------------------------------ model

def _factor_arrays(block):
    n = len(block)
    starts = np.asarray(O.duval_starts(block), np.int64)
    ends = np.append(starts[1:], n)
    fid = np.repeat(np.arange(len(starts)), ends - starts)
    return starts[fid], (ends - starts)[fid]  # per position: factor start, factor length


def _group_starts(keys):
    """For sorted keys (one array, or several compared in turn): per index the index at which its
    run of equal keys starts."""
    keys = keys if isinstance(keys, (list, tuple)) else [keys]
    n = len(keys[0])
    head = np.zeros(n, bool)
    head[:1] = True
    for k in keys:
        head[1:] |= k[1:] != k[:-1]
    idx = np.arange(n, dtype=np.int64)
    return np.maximum.accumulate(np.where(head, idx, 0))


def rotation_classes(block, nchars):
    """The classes of positions whose rotations agree on nchars characters, by sorting the
    prefixes themselves (the brute force the model is tested against): per position the number
    of positions with a smaller prefix, which is the rank the model keeps."""
    t = np.frombuffer(block, np.uint8)
    fs, m = _factor_arrays(block)
    p = np.arange(len(block), dtype=np.int64)
    rows = [bytes(t[fs[i] + (i - fs[i] + np.arange(nchars)) % m[i]]) for i in p]
    order = sorted(p.tolist(), key=lambda i: rows[i])
    rank = np.zeros(len(block), np.int64)
    start = 0
    for j, i in enumerate(order):
        if j and rows[i] != rows[order[j - 1]]:
            start = j
        rank[i] = start
    return rank


class BlockModel:
    """The doubling rounds of one block.  State as on the device: rk[p] = number of positions of
    the block whose rotation is smaller on the characters compared so far (the start of p's group
    in the sorted order), so equal rk = one group, and round r sorts every group of two or more
    by rk[succ^h(p)], h = 8 * 2^(r-1).

    rounds[r - 1] for round r = 1, 2, ... while the block is live: dict(active, hist, sizes,
    longest, bucket, large, starts, lens) - hist[k] groups of class k (index NCLASS: larger than
    TILE), sizes {group size: count}, the longest group, the largest group left after the round's
    refinement (a bucket of equal keys: this round could not split it), large = the round's keys
    of every group larger than TILE (one array per group), and every group's first slot in the
    block's sorted order with its length.  last_split: the last round (0 = round 0)
    that split one of the block's groups.  ranks[r]: rk after round r (kept on request).
    A block retires with the ranks final: a round that splits nothing has reached the fixed point."""

    def __init__(self, block, keep_ranks=False):
        t = np.frombuffer(block, np.uint8)
        n = len(t)
        fs, m = _factor_arrays(block)
        p = np.arange(n, dtype=np.int64)
        key = np.zeros(n, np.uint64)
        for k in range(H0):  # the first 8 characters of every rotation, the first most significant
            key = (key << np.uint64(8)) | t[fs + (p - fs + k) % m].astype(np.uint64)
        order = np.argsort(key, kind="stable")
        rk = np.empty(n, np.int64)
        rk[order] = _group_starts(key[order])
        self.n = n
        self.distinct = len(np.unique(t))
        self.rounds = []
        self.last_split = 0
        self.ranks = [rk.copy()] if keep_ranks else None
        live = bool(rk.max() > 0) if n else False  # round 0 split the block
        h = H0
        while live:
            cnt = np.bincount(rk, minlength=n)
            act = np.flatnonzero(cnt[rk] >= 2)  # positions in groups of two or more
            if act.size == 0:
                break
            k1 = rk[act]
            k2 = rk[fs[act] + (act - fs[act] + h) % m[act]]
            o = np.lexsort((k2, k1))
            k1, k2, act = k1[o], k2[o], act[o]
            old = _group_starts(k1)
            new = _group_starts([k1, k2])
            gsz = cnt[cnt >= 2]
            sizes, mult = np.unique(gsz, return_counts=True)
            hist = [0] * (NCLASS + 1)
            for g, c in zip(sizes.tolist(), mult.tolist()):
                hist[size_class(g) if g <= TILE else NCLASS] += c
            heads = np.flatnonzero(old == np.arange(len(old)))
            large = [k2[s:s + cnt[k1[s]]] for s in heads if cnt[k1[s]] > TILE]
            nrk = k1 + (new - old)
            self.rounds.append(dict(active=int(act.size), hist=hist, sizes=dict(zip(sizes.tolist(), mult.tolist())),
                                    longest=int(gsz.max()), bucket=int(np.bincount(nrk).max()), large=large,
                                    starts=k1[heads], lens=cnt[k1[heads]]))
            live = bool((new != old).any())
            if live:
                self.last_split = len(self.rounds)
            rk[act] = nrk
            if keep_ranks:
                self.ranks.append(rk.copy())
            h *= 2
        self._t, self._fs, self._m, self._rk = t, fs, m, rk

    def bbwt(self):
        """The BBWT of the block from the final ranks: the positions in rank order, ties (the
        rotations that never differ) in position order, each giving its cyclic predecessor's byte."""
        order = np.lexsort((np.arange(self.n), self._rk))
        fs, m = self._fs[order], self._m[order]
        return self._t[fs + (order - fs + m - 1) % m].tobytes()


@functools.lru_cache(maxsize=512)
def block_model(block):
    return BlockModel(block)


def model_payload(block):
    """The method-2 payload (BBWT -> MTF -> Rice, k = 2) from the model's order, with the oracle's
    MTF and Rice coders: what the oracle's candidate 2 is, without its BBWT (seconds on long
    repetitive blocks)."""
    return O.rice_encode(O.mtf_encode(block_model(block).bbwt()), 2)


def msd_round(large, key_bits, med):
    """What sort_pass does with a round's groups larger than TILE (`large`: their keys).
    Returns dict(levels, medium, eq, added): MSD levels run, launches of the medium sort, buckets
    finished as equal-key runs, and added[k] = buckets of class k that the levels append to the
    class lists (k = 0: single elements).

    med (batches under 64 blocks): if no group is longer than MED_T, one medium-sort launch takes
    them all; otherwise every level is preceded by a medium-sort launch that takes the level's
    segments of at most MED_T elements.  A level splits a segment by the next digit of the key (8
    bits from the top of key_bits, the last level narrower): a bucket of at most TILE elements
    joins its class list, a larger one goes to the next level, or after the last digit is an
    equal-key run."""
    out = dict(levels=0, medium=0, eq=0, added=[0] * NCLASS)
    if not large:
        return out
    if med and max(len(g) for g in large) <= MED_T:
        out["medium"] = 1
        return out
    segs = list(large)
    hi = key_bits
    while hi:
        width = min(8, hi)
        shift = hi - width
        out["levels"] += 1
        out["medium"] += 1 if med else 0
        nxt = []
        for g in segs:
            if med and len(g) <= MED_T:
                continue  # the medium sort took it
            digit = (g >> shift) & ((1 << width) - 1)
            for d in np.unique(digit):
                b = g[digit == d]
                if len(b) <= TILE:
                    out["added"][size_class(len(b))] += 1
                elif shift:
                    nxt.append(b)
                else:
                    out["eq"] += 1
        segs = nxt  # (the host runs every level whether or not segments are left)
        hi = shift
    return out


class BatchModel:
    """The rounds of a batch of blocks: per round the sums (active, hist, sizes), the maxima
    (longest, bucket), the large groups' keys and every group's first slot in the batch's sorted
    array (starts, with lens) over the blocks still live.  cyc_active /
    cyc_rounds / rounds_sum: what the device reports in kolm_stats for the batch in the fixed
    8-bit form (N positions for round 0 plus the rounds' active counts; 1 + rounds; the sum over
    blocks of the last splitting round + 1)."""

    def __init__(self, blocks):
        bm = [block_model(b) for b in blocks]
        self.N = sum(len(b) for b in blocks)
        self.nb = len(blocks)
        self.bs = max(len(b) for b in blocks)
        self.blocks = bm
        self.rounds = []
        base = np.concatenate([[0], np.cumsum([len(b) for b in blocks])])
        for r in range(max((len(x.rounds) for x in bm), default=0)):
            rs = [x.rounds[r] for x in bm if len(x.rounds) > r]
            at = [base[i] for i, x in enumerate(bm) if len(x.rounds) > r]
            sizes = {}
            for x in rs:
                for g, c in x["sizes"].items():
                    sizes[g] = sizes.get(g, 0) + c
            self.rounds.append(dict(active=sum(x["active"] for x in rs),
                                    hist=[sum(x["hist"][k] for x in rs) for k in range(NCLASS + 1)],
                                    sizes=sizes, longest=max(x["longest"] for x in rs),
                                    bucket=max(x["bucket"] for x in rs), large=[g for x in rs for g in x["large"]],
                                    starts=np.concatenate([x["starts"] + b for x, b in zip(rs, at)]),
                                    lens=np.concatenate([x["lens"] for x in rs])))
        self.cyc_active = self.N + sum(r["active"] for r in self.rounds)
        self.cyc_rounds = 1 + len(self.rounds)
        self.rounds_sum = sum(x.last_split + 1 for x in bm)
        # 8-bit fixed codes: the widest alphabet of the batch needs 8 bits
        self.fixed_8bit = 129 <= max(x.distinct for x in bm) <= 256

    def dense(self, r):
        """Round r (1-based) is a dense round: more than 1/8 of the batch's positions active."""
        return self.rounds[r - 1]["active"] * 8 > self.N

    def groups(self, r, size):
        """Groups of exactly `size` elements in round r (0 past the last round)."""
        return self.rounds[r - 1]["sizes"].get(size, 0) if r <= len(self.rounds) else 0

    def launches(self):
        """Launch count per kernel name of the doubling rounds, as sort_pass records them, in the
        fixed 8-bit form."""
        med = self.nb < 64
        rank_bits = max(bitlen(self.bs), 1)       # digits of the MSD levels
        key_bits = bitlen(self.bs - 1)            # sort-word width of the LDS sorts
        out = {}

        def add(name, k=1):
            out[name] = out.get(name, 0) + k
        add("k_classify", self.cyc_rounds)  # every round, and the one that finds nothing active
        for r, x in enumerate(self.rounds, 1):
            dense = self.dense(r)
            if dense:
                add("k_keypos")
            if any(x["hist"][k] for k in range(1 if not dense else 5, NCLASS)):
                add("k_keygen_small")
            m = msd_round(x["large"], rank_bits, med)
            if x["large"]:
                add("k_keygen_large")
            add("k_small_sort<13> (medium)", m["medium"])
            for nm in ("k_msd_hist", "k_msd_scan", "k_msd_scatter", "k_copy_back"):
                add(nm, m["levels"])
            cls = [x["hist"][k] + m["added"][k] for k in range(NCLASS)]
            if cls[0]:
                add("k_single")
            for k in range(1, 5):
                if cls[k]:
                    add(f"k_tiny_sort<{k}>")
            if any(cls[k] and key_bits + k <= 31 for k in range(5, NCLASS)):
                add("k_small_sort_all<u32>")
            if any(cls[k] and key_bits + k > 31 for k in range(5, NCLASS)):
                add("k_small_sort_all<u64>")
            if m["eq"]:
                add("k_finalize_eq")
        return {k: v for k, v in out.items() if v}


SORT_KERNELS = ("k_single", "k_tiny_sort<1>", "k_tiny_sort<2>", "k_tiny_sort<3>", "k_tiny_sort<4>",
                "k_small_sort_all<u32>", "k_small_sort_all<u64>", "k_small_sort<13> (medium)", "k_msd_hist",
                "k_msd_scan", "k_msd_scatter", "k_copy_back", "k_finalize_eq", "k_keypos", "k_keygen_small",
                "k_keygen_large", "k_classify")


# ------------------------------------------------------------------ the route matrix

HOT, DEFAULT = 0x1FF, 0x3FF  # candidate masks: the hot path (ids 0..8), and with Re-Pair (id 9)

TINY_G = (2, 3, 4, 5, 8, 9, 16)
SMALL_G1 = (17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513)
SMALL_G2 = (1024, 1025, 2048)
EARLY_G = (40, 200, 600, 3000)
ORACLE_MAX = 200_000  # blocks up to this size are compared with the oracle (longer: its BBWT takes seconds)


def spread(case_blocks, nb, seed=900):
    """A batch of nb blocks: the case blocks at even distances from the first block to the last,
    tiny blocks in between."""
    k = len(case_blocks)
    at = {round(i * (nb - 1) / max(k - 1, 1)): b for i, b in enumerate(case_blocks)} if k > 1 else {nb // 2: case_blocks[0]}
    assert len(at) == k and nb >= k
    return [at.get(i) or small_block(seed + i, 96 + i % 7) for i in range(nb)]


def _fam_blocks(gs, L, seed, lead=True, filler=0):
    return build_block(seed, [(g, L) for g in gs], lead=lead, filler=filler, split=not lead)


@functools.lru_cache(maxsize=None)
def _medium():
    return [build_block(g, [(g, 17)]) for g in (2049, 4096, 8192)]


@functools.lru_cache(maxsize=None)
def _early():
    return [build_block(10 + g, [(g, 300)]) for g in EARLY_G]


def _retire():
    out = []
    for i in range(10):
        out += [periodic_block(40 + i, 300, 20), build_block(60 + i, [(40, 300)])]
    return out


class Case:
    """One row of the matrix: make() builds the batch's blocks; mask: the candidate mask of the
    route run."""

    def __init__(self, name, make, mask=HOT):
        self.name, self.make, self.mask = name, make, mask

    @functools.lru_cache(maxsize=None)
    def blocks(self):
        return tuple(self.make())

    def model(self):
        return BatchModel(self.blocks())


def _cases():
    c = []

    def add(name, make, mask=HOT):
        c.append(Case(name, make, mask))
    for nb in (3, 20, 64):
        add(f"tiny_dense_nb{nb}", lambda nb=nb: [_fam_blocks(TINY_G, 40, 100 + i) for i in range(nb)])
    for nb in (3, 20):
        add(f"tiny_sparse_nb{nb}", lambda nb=nb: [_fam_blocks(TINY_G, 40, 200 + i, filler=30000) for i in range(nb)])
    small = lambda: [_fam_blocks(SMALL_G1, 24, 2), _fam_blocks(SMALL_G2, 24, 3)]  # noqa: E731
    add("small_dense_nb3", lambda: small() + [small_block(5)])
    add("small_dense_nb20", lambda: spread(small(), 20))
    add("small_dense_nb64", lambda: spread(small(), 64))
    sparse = lambda: [_fam_blocks(SMALL_G1, 12, 6, filler=150000), _fam_blocks(SMALL_G2, 12, 7),  # noqa: E731
                      build_block(8, [], filler=190000)]
    add("small_sparse_nb3", sparse)
    add("small_sparse_nb20", lambda: spread(sparse(), 20))
    add("medium_nb3", _medium)
    add("medium_nb20", lambda: spread(_medium(), 20))
    add("msd_moderate_nb64", lambda: spread(_medium(), 64))
    for bs in (65535, 65536, 65537):
        add(f"msd_levels_bs{bs}", lambda bs=bs: spread([build_block(5, [Fam(2100, 28, pin=True)], length=bs)], 64))
    add("mixed_medium_msd_nb3", lambda: [build_block(8193, [(8193, 17)]), build_block(3000, [(3000, 17)]), small_block(9)])
    add("equal_runs_nb3", lambda: spread([build_block(6, [Fam(9000, 17, two=True)])], 3))
    add("equal_runs_nb64", lambda: spread([build_block(7, [Fam(5000, 17, two=True)])], 64))
    add("equal_runs_over_medium_nb3", lambda: spread([build_block(8, [Fam(18000, 16, two=True)])], 3))
    add("u64_words", lambda: [build_block(9, [(1500, 40), (700, 40)], length=(1 << 20) + 1), small_block(10)])
    add("early_gather_nb20", lambda: spread(_early(), 20))
    add("early_gather_nb64", lambda: spread(_early(), 64))
    add("early_off_repair_nb20", lambda: spread(_early(), 20), DEFAULT)
    add("early_off_nb3", lambda: _early()[:3])
    add("retire_nb20", _retire)
    add("multi_factor_tiny_nb3", lambda: [_fam_blocks(TINY_G, 40, 300 + i, lead=False) for i in range(3)])
    add("multi_factor_small_nb3", lambda: [_fam_blocks(SMALL_G1, 24, 12, lead=False),
                                           _fam_blocks(SMALL_G2, 24, 13, lead=False), small_block(14)])
    return {x.name: x for x in c}


CASES = _cases()
