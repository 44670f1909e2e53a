"""Built systems for the sparse block search (k_block_sparse) and what each must trigger (inputs only -- no solver here).

The test, not chance, decides what the kernel sees.  A row whose support lies inside ONE 64-column panel (plus the constant) is never
changed by the elimination of another panel and causes no fill-in, so a system made of such rows is block-diagonal by panel and the
window k_block_sparse meets at block b is exactly what was written here.  Its pool is the alive rows with a non-zero window in row
order: the rows written for the block's four panels, in the order they were written.  Depth in the pool, the rank of the first 64 and
the first 512 entries of a panel and the rank of the truncated pool on a panel can therefore be read off the construction with an
integer echelon basis (`rank_of`), and `predict` walks the branches of the kernel and of the host's hand-backs (hand_back: probed, or met after submission) over them.

Every case carries the counters it expects (gf2bv_stats::sparse_*): `("==", v)` where the construction fixes the value, `(">=", v)`
where it only bounds it.  tests/test_sparse_cases_cpu.py checks the preconditions and that `predict` arrives at the exact ones;
tests/test_gpu_sparse_search.py runs the cases."""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

POOLS = (1024, 4096, 6144)      # kSparsePools, by ForwardRun::tier: k_block_sparse<256, 4> / <512, 8> / <1024, 6>, NT x CPT candidates
SP_NE = 512                     # GF2_SP_NE: entries of a panel that selection (A) looks at
SP_NW = 1024                    # GF2_SP_NW: mask words (of 64 rows) the pool is gathered from, counted from the alive bound's word
NZ_LARGEST = 3400               # forward_block: `hst.sp_nz > 3400` on a probed block sends the blocks behind it to the largest pool
CYCLE = 8                       # SolveState::sp_chunk `& 7`: after a miss of (A) seven blocks go straight to the rounds (B)
STRIKES = 3                     # hand_back: the third give-up of a solve switches the search off
FAST_NC = 320                   # GF2_FAST_NC: rows a system needs for any one-launch search (fast_block_possible)
MIN_BLOCKS = 8                  # forward_block: the look at block 0 wants `nblocks >= 8`
G = 4                           # GF2_GMAX: panels of a block
DENSE_WORDS, DENSE_BITS = 48, 12      # k_block_fast: it takes a panel when 48 of the 64 candidate words have more than 12 bits
TWO_LEVEL_MIN_BYTES = 1 << 29   # plan_two_level: `min_bytes = 0.5 * 1073741824.0` of trailing matrix before outer panels are planned

M64 = (1 << 64) - 1


def rank_of(words) -> int:
    """rank over GF(2) of 64-bit words (echelon basis by highest bit)"""
    basis = {}
    for w in words:
        while w:
            h = w.bit_length() - 1
            if h not in basis:
                basis[h] = w
                break
            w ^= basis[h]
    return len(basis)


def independent_words(rng: random.Random, n: int = 64) -> list:
    """n <= 64 independent random 64-bit words"""
    out = []
    while len(out) < n:
        w = rng.getrandbits(64)
        if rank_of(out + [w]) == len(out) + 1:
            out.append(w)
    return out


def copies(rng: random.Random, span: list, n: int) -> list:
    """n non-zero combinations of two or three of the independent words `span`: rows that add nothing to their rank"""
    out = []
    for _ in range(n):
        w = 0
        for v in rng.sample(span, min(len(span), rng.choice((2, 3)))):
            w ^= v
        out.append(w)
    return out


# ---- a block's rows: lists of (panel within the block, word), in row order ---------------------------------------------------------

def easy_block(rng, extra: int = 16) -> list:
    """panel after panel: 64 independent rows, then `extra` copies.  The first 64 entries of every panel are independent."""
    rows = []
    for g in range(G):
        b = independent_words(rng)
        rows += [(g, w) for w in b + copies(rng, b, extra)]
    return rows


def absorb_block(rng, g: int, entry: int, extra: int = 16) -> list:
    """like easy_block, but panel g: 63 independent rows, copies of them, and the row that completes the panel as entry `entry`
    (0-based, among the rows that carry a bit in panel g) -- the first 64 entries have rank 63 whatever follows"""
    assert entry >= 64
    rows = []
    for q in range(G):
        b = independent_words(rng)
        if q == g:
            rows += [(q, w) for w in b[:63] + copies(rng, b[:63], entry - 63) + [b[63] ^ b[0]] + copies(rng, b, extra)]
        else:
            rows += [(q, w) for w in b + copies(rng, b, extra)]
    return rows


def deep_block(rng, depth: int, g: int = 3, extra: int = 16) -> list:
    """the other panels easy and in front; panel g: 63 independent rows, copies, and its 64th independent row as pool row `depth` (0-based)
    -- a pool of `depth` rows or fewer has rank 63 on panel g"""
    rows = []
    bases = [independent_words(rng) for _ in range(G)]
    for q in range(G):
        if q != g:
            rows += [(q, w) for w in bases[q] + copies(rng, bases[q], extra)]
    b = bases[g]
    rows += [(g, w) for w in b[:63]]
    assert depth - len(rows) >= SP_NE, "the completing row must lie behind the entries (A) looks at, too"
    rows += [(g, w) for w in copies(rng, b[:63], depth - len(rows))]
    rows += [(g, b[63] ^ b[1])]
    assert rows[depth] == (g, b[63] ^ b[1])
    return rows


def front_loaded_block(rng, tail: int) -> list:
    """the four panels' 64 independent rows first (256 rows), then `tail` copies of all four: a long pool whose pivots are in front"""
    bases = [independent_words(rng) for _ in range(G)]
    rows = [(g, w) for g in range(G) for w in bases[g]]
    rows += [(i % G, copies(rng, bases[i % G], 1)[0]) for i in range(tail)]
    return rows


def deficient_block(rng, g: int = 1, extra: int = 40) -> list:
    """panel g has rank 63 over all its rows (64 + extra of them): no pool completes it.  The others are easy."""
    rows = []
    for q in range(G):
        b = independent_words(rng)
        if q == g:
            rows += [(q, w) for w in b[:63] + copies(rng, b[:63], extra + 1)]
        else:
            rows += [(q, w) for w in b + copies(rng, b, extra)]
    return rows


def short_panel_block(rng, g: int = 2, have: int = 40, extra: int = 50) -> list:
    """panel g has only `have` < 64 rows that carry a bit in it (independent); the block still has more than 256 rows"""
    rows = []
    for q in range(G):
        b = independent_words(rng)
        rows += [(q, w) for w in (b[:have] if q == g else b + copies(rng, b, extra))]
    return rows


def thin_block(rng, per_panel: int = 60) -> list:
    """4 x per_panel < 256 rows in all: fewer candidates than the block has pivots"""
    rows = []
    for q in range(G):
        rows += [(q, w) for w in independent_words(rng, per_panel)]
    return rows


def dup_front_block(rng, extra: int = 16) -> list:
    """every panel: a row, its copy right behind it, then the other 63 independent rows and `extra` copies.  The copy is a pool row
    that is never taken and lies above nearly all the rows that are (min_free), and it makes the first 64 entries one short."""
    rows = []
    for g in range(G):
        b = independent_words(rng)
        rows += [(g, w) for w in [b[0], b[0]] + b[1:] + copies(rng, b, extra)]
    return rows


# ---- a system ----------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    cols: int
    layout: list                   # row order: ("block", b) = the rows of blocks[b], ("zero", n) = n all-zero rows, ("plain", [ints]) = ordinary rows
    blocks: dict                   # block index -> [(panel within the block, word)]
    expect: dict                   # counter (or "counter[i]") -> (op, value)
    consistent: bool = True
    seed: int = 0
    modes: tuple = (0, 1)
    diagonal: bool = True          # only panel-confined rows: `predict` applies
    note: str = ""
    _built: dict = field(default_factory=dict, repr=False)

    @property
    def full_blocks(self) -> int:
        return self.cols // (64 * G)

    def coefficient_rows(self) -> list:
        """[(panel, word) | None (zero row) | int (ordinary row's coefficients)] in row order"""
        out = []
        for kind, what in self.layout:
            if kind == "block":
                out += [(G * what + g, w) for g, w in self.blocks[what]]
            elif kind == "zero":
                out += [None] * what
            else:
                out += list(what)
        return out

    def aug(self) -> np.ndarray:
        """the packed augmented matrix (rows x words, column `cols` = constant), constants from a planted solution; an inconsistent
        case has the constants of three rows that are combinations of others flipped"""
        if "aug" not in self._built:
            rows = self.coefficient_rows()
            wt = (self.cols + 1 + 63) // 64
            rng = random.Random(self.seed ^ 0x5EED)
            plant = [rng.getrandbits(64) for _ in range(wt)]
            a = np.zeros((len(rows), wt), dtype=np.uint64)
            const = np.zeros(len(rows), dtype=np.uint64)
            for i, r in enumerate(rows):
                if r is None:
                    continue
                if isinstance(r, tuple):
                    a[i, r[0]] = r[1]
                    const[i] = bin(r[1] & plant[r[0]]).count("1") & 1
                else:
                    for q in range(wt):
                        w = (r >> (64 * q)) & M64
                        a[i, q] = w
                        const[i] ^= bin(w & plant[q]).count("1") & 1
            if not self.consistent:
                for i in self.redundant_rows()[:3]:
                    const[i] ^= np.uint64(1)
            a[:, self.cols // 64] |= const << np.uint64(self.cols % 64)
            self._built["aug"] = a
        return self._built["aug"]

    def redundant_rows(self) -> list:
        """rows (panel-confined) that are combinations of earlier rows of their panel"""
        seen, out = {}, []
        for i, r in enumerate(self.coefficient_rows()):
            if isinstance(r, tuple):
                have = seen.setdefault(r[0], [])
                if rank_of(have + [r[1]]) == len(have):
                    out.append(i)
                else:
                    have.append(r[1])
        return out

    def rank(self) -> int:
        """of a diagonal case: the sum of its panels' ranks"""
        assert self.diagonal
        by = {}
        for r in self.coefficient_rows():
            if r is not None:
                by.setdefault(r[0], []).append(r[1])
        return sum(rank_of(v) for v in by.values())

    def block_start(self, b: int) -> int:
        at = 0
        for kind, what in self.layout:
            if (kind, what) == ("block", b):
                return at
            at += len(self.blocks[what]) if kind == "block" else what if kind == "zero" else len(what)
        raise KeyError(b)

    def check_preconditions(self) -> None:
        """what forward_block and block_way want before they let k_block_sparse at a block"""
        rows = self.coefficient_rows()
        aug = self.aug()
        assert aug.ndim == 2 and aug.shape[0] == len(rows), "a single system: one rows x words matrix (a gang never takes the search)"
        # not two-level: plan_two_level plans no outer panel while the matrix behind it would be smaller than min_bytes, and the
        # whole matrix is
        assert aug.shape[0] * aug.shape[1] * 8 < TWO_LEVEL_MIN_BYTES, "a one-level plan"
        assert self.cols % 64 == 0 and 2304 <= self.cols <= 3072
        assert (self.cols + 1 + 63) // 64 >= G * MIN_BLOCKS, "at least 8 blocks"
        assert len(rows) >= FAST_NC
        for b in self.blocks:
            assert 0 <= b < self.full_blocks and (G * b + G) * 64 <= self.cols, "every built block is a full one"
        # block 0: the dense search looks at panel 0's words of the first 64 rows and declines
        dense = sum(1 for r in rows[:64] if isinstance(r, tuple) and r[0] == 0 and bin(r[1]).count("1") > DENSE_BITS)
        dense += sum(1 for r in rows[:64] if isinstance(r, int) and bin(r & M64).count("1") > DENSE_BITS)
        assert dense < DENSE_WORDS, "the dense search must refuse block 0"


def predict(case: Case) -> dict:
    """The branches k_block_sparse and the host's hand-backs (probed, or met after submission) take over a diagonal case, from ranks and depths alone: the counters
    of gf2bv_stats::sparse_* and, per block, what happened ("trace")."""
    assert case.diagonal
    st = {"sparse_blocks": [0, 0, 0], "sparse_panels_first64": 0, "sparse_panels_absorb": 0, "sparse_panels_rounds": 0,
          "sparse_giveups": 0, "sparse_giveup_why": [0] * 5, "sparse_nz_max": 0, "trace": []}
    # The mask words in reach: SP_NW words from the alive bound's word on.  The bound is never above a row that stays alive, so never
    # above the first all-zero row: a row below 64 * SP_NW is in reach whatever the bound, a row at or above `far` is out of reach
    layout_rows = case.coefficient_rows()
    never_pivot = next((i for i, r in enumerate(layout_rows) if r is None), len(layout_rows))
    near, far = 64 * SP_NW, (never_pivot // 64 + SP_NW) * 64
    tier, probes, on, sp_chunk = 0, 1, True, 0
    for b in range(1, case.full_blocks):
        if not on:
            st["trace"].append((b, "general"))
            continue
        rows = case.blocks.get(b, [])
        start = case.block_start(b) if b in case.blocks else 0
        assert all(start + i < near or start + i >= far for i in range(len(rows))), "a row that may or may not be in reach decides nothing"
        pool_all = [r for i, r in enumerate(rows) if start + i < near]
        st["sparse_nz_max"] = max(st["sparse_nz_max"], len(pool_all))
        pool = pool_all[:POOLS[tier]]
        why, how = 0, []
        if len(pool) < 64 * G:
            why = 2
        try_chunk = sp_chunk == 0
        for g in range(G):
            if why:
                break
            entries = [w for q, w in pool if q == g]
            done = False
            if try_chunk:
                if len(entries) < 64:
                    why = 5
                    break
                if rank_of(entries[:64]) == 64:
                    how.append("first64")
                    done = True
                elif rank_of(entries[:SP_NE]) == 64:
                    how.append("absorb")
                    done = True
                try_chunk = done
            if not done:
                if rank_of(entries) < 64:
                    why = 3
                    break
                how.append("rounds")
        probed = probes > 0
        probes -= probed
        want = 2 if len(pool_all) > NZ_LARGEST else 0
        if why:
            st["sparse_giveups"] += 1
            st["sparse_giveup_why"][why - 1] += 1
            on = st["sparse_giveups"] < STRIKES
            st["trace"].append((b, f"pool {tier} gives up: reason {why}, {'probed' if probed else 'pipelined'}"))
            if probed:
                probes = 1 if on else 0
                tier = min(2, max(tier + 1, want))
            else:
                tier = min(2, tier + 1)
        else:
            st["sparse_blocks"][tier] += 1
            for h in how:
                st["sparse_panels_" + h] += 1
            st["trace"].append((b, f"pool {tier}: {' '.join(how)}"))
            sp_chunk = 0 if try_chunk else (sp_chunk + 1) % CYCLE
            if probed:
                tier = max(tier, want)
    return st


def _std_layout(blocks: dict, order=None) -> list:
    """block 0's rows (the general steps take them) go last unless placed, so that the first 64 rows have no bit in panel 0"""
    order = list(order) if order is not None else [b for b in sorted(blocks) if b != 0]
    if 0 not in order:
        order.append(0)
    return [("block", b) for b in order]


def _case(name, cols, seed, make, expect, order=None, layout=None, **kw) -> Case:
    rng = random.Random(seed)
    nb = cols // (64 * G)
    blocks = {0: easy_block(rng)}
    for b in range(1, nb):
        blocks[b] = make(b, rng)
    return Case(name, cols, layout(blocks) if layout else _std_layout(blocks, order), blocks, expect, seed=seed, **kw)


def eq(v):
    return ("==", v)


def ge(v):
    return (">=", v)


NO_GIVEUP = {"sparse_giveups": eq(0), "sparse_giveup_why": eq([0] * 5)}


def _plain_rows(rng, n, cols, bits):
    out = []
    for _ in range(n):
        a = 0
        for _ in range(bits):
            a |= 1 << rng.randrange(cols)
        out.append(a)
    return out


def _shuffled(name, seed, bits, plain) -> Case:
    """panel-confined rows mixed with ordinary sparse rows and shuffled: later panels see fill-in.  No prediction: counters only >=."""
    rng = random.Random(seed)
    cols = 2304
    blocks = {b: easy_block(rng, extra=24) for b in range(cols // (64 * G))}
    rows = [(G * b + g, w) for b, blk in blocks.items() for g, w in blk]
    mixed = [w << (64 * p) for p, w in rows] + _plain_rows(rng, plain, cols, bits)
    rng.shuffle(mixed)
    # (the first 64 rows are sparse in panel 0 whatever the shuffle brings: at most one row in nine has a word there at all)
    return Case(name, cols, [("plain", mixed)], {}, {"sparse_blocks_sum": ge(1)}, seed=seed, diagonal=False,
                note="shuffled, with fill-in from ordinary rows")


def _two_block_row_case() -> Case:
    rng = random.Random(94)
    cols, col, late, g = 2304, 7, 5, 2
    blocks = {b: easy_block(rng) for b in range(cols // (64 * G))}
    # block `late`, panel g: 63 independent rows without a bit in column `col` (and copies of them) -- rank 63 on their own
    b = []
    while len(b) < 63:
        w = rng.getrandbits(64) & ~(1 << col)
        if rank_of(b + [w]) == len(b) + 1:
            b.append(w)
    others = [r for r in blocks[late] if r[0] != g]
    blocks[late] = others[:2 * 80] + [(g, w) for w in b + copies(rng, b, 16)] + others[2 * 80:]
    head = blocks[1][0]
    assert head[0] == 0
    first = head[1] << (64 * (G * 1 + 0))
    both = first | (((1 << col) | b[3]) << (64 * (G * late + g)))
    blocks[1] = blocks[1][1:]
    layout = [("plain", [first, both])] + [("block", q) for q in range(1, cols // (64 * G))] + [("block", 0)]
    return Case("alive_min_free_row_in_two_blocks", cols, layout, blocks,
                {"sparse_blocks": eq([8, 0, 0]), "sparse_panels_first64": eq(31), "sparse_panels_absorb": eq(1),
                 "sparse_panels_rounds": eq(0), **NO_GIVEUP}, seed=94, diagonal=False,
                note="row 1 has support in blocks 1 and 5; counters by hand: block 1 panel 0 meets a copy among its first 64 entries "
                     "(find_absorb), block 5 panel 2 has row 1 as its first entry and 63 independent rows behind it")


def all_cases() -> list:
    C = []
    # first64: every panel's first 64 entries independent
    C.append(_case("first64", 2304, 11, lambda b, r: easy_block(r),
                   {"sparse_blocks": eq([8, 0, 0]), "sparse_panels_first64": eq(32), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), "sparse_nz_max": eq(320), **NO_GIVEUP}))
    # absorb: copies in front, the completing row inside the first 512 entries / as entry 511 / as entry 512
    for name, entry, exp in (("absorb_100", 100, (31, 1, 0)), ("absorb_511", 511, (31, 1, 0)), ("absorb_512", 512, (2, 0, 30))):
        C.append(_case(name, 2304, 20 + entry, lambda b, r, e=entry: absorb_block(r, 2, e) if b == 1 else easy_block(r),
                       {"sparse_blocks": eq([8, 0, 0]), "sparse_panels_first64": eq(exp[0]), "sparse_panels_absorb": eq(exp[1]),
                        "sparse_panels_rounds": eq(exp[2]), **NO_GIVEUP}))
    # the cycle: block 1 misses (A) on its first panel, blocks 2..8 run (B) untried although (A) would succeed, block 9 tries again (and
    # needs find_absorb), blocks 10 and 11 stay on (A)
    C.append(_case("cycle", 3072, 31, lambda b, r: absorb_block(r, 0, 512) if b == 1 else absorb_block(r, 1, 100) if b == 9 else easy_block(r),
                   {"sparse_blocks": eq([11, 0, 0]), "sparse_panels_first64": eq(11), "sparse_panels_absorb": eq(1),
                    "sparse_panels_rounds": eq(32), **NO_GIVEUP}))
    # truncated pool: 1456 rows with a non-zero window, the pivots inside the first 1024
    C.append(_case("truncated", 2304, 41, lambda b, r: front_loaded_block(r, 1200) if b in (1, 4) else easy_block(r),
                   {"sparse_blocks": eq([8, 0, 0]), "sparse_panels_first64": eq(32), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), "sparse_nz_max": eq(1456), **NO_GIVEUP}))
    # probed escalation: the 64th independent row of a panel 1500 deep -- reason 3 on the small pool, the middle pool completes the next
    # block built the same way (by the rounds: (A) misses there too, so the blocks behind it go to the rounds)
    C.append(_case("escalate_middle", 2304, 51, lambda b, r: deep_block(r, 1500) if b in (1, 2) else easy_block(r),
                   {"sparse_blocks": eq([0, 7, 0]), "sparse_panels_first64": eq(3), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(25), "sparse_giveups": eq(1), "sparse_giveup_why": eq([0, 0, 1, 0, 0]),
                    "sparse_nz_max": eq(1501)}))
    # ... 5000 deep from there on: the middle pool gives up as well (probed: it is the first block of its size), the largest completes
    C.append(_case("escalate_largest", 2304, 52, lambda b, r: deep_block(r, 1500) if b == 1 else deep_block(r, 5000) if b in (2, 3) else easy_block(r),
                   {"sparse_blocks": eq([0, 0, 6]), "sparse_panels_first64": eq(3), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(21), "sparse_giveups": eq(2), "sparse_giveup_why": eq([0, 0, 2, 0, 0]),
                    "sparse_nz_max": eq(5001)}))
    # more than 3400 rows with a non-zero window on the first sparse block, no give-up: straight to the largest pool
    C.append(_case("straight_to_largest", 2304, 53, lambda b, r: front_loaded_block(r, 3300) if b == 1 else easy_block(r),
                   {"sparse_blocks": eq([1, 0, 7]), "sparse_panels_first64": eq(32), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), "sparse_nz_max": eq(3556), **NO_GIVEUP}))
    # ... and 5000 deep on the probed block itself: the small pool gives up having counted more than NZ_LARGEST rows, and the search
    # skips the middle pool (a probed hand-back raises the pool to max(next, wanted), not by one)
    C.append(_case("escalate_skip_middle", 2304, 54, lambda b, r: deep_block(r, 5000) if b in (1, 2) else easy_block(r),
                   {"sparse_blocks": eq([0, 0, 7]), "sparse_panels_first64": eq(3), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(25), "sparse_giveups": eq(1), "sparse_giveup_why": eq([0, 0, 1, 0, 0]),
                    "sparse_nz_max": eq(5001)}))
    # pipelined resume: blocks 1..4 easy, block 5 needs depth 1500 -- found after everything was submitted; the middle pool behind it
    C.append(_case("pipelined", 2304, 61, lambda b, r: deep_block(r, 1500) if b == 5 else easy_block(r),
                   {"sparse_blocks": eq([4, 3, 0]), "sparse_panels_first64": eq(28), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), "sparse_giveups": eq(1), "sparse_giveup_why": eq([0, 0, 1, 0, 0])}))
    # ... 5000 deep, twice: a hand-back found after submission raises the pool by one whatever was counted, so block 5 brings the
    # middle pool, block 6 gives up on that one (pipelined again: no probe is re-armed) and brings the largest -- two give-ups
    C.append(_case("pipelined_deep", 2304, 62, lambda b, r: deep_block(r, 5000) if b in (5, 6) else easy_block(r),
                   {"sparse_blocks": eq([4, 0, 2]), "sparse_panels_first64": eq(24), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), "sparse_giveups": eq(2), "sparse_giveup_why": eq([0, 0, 2, 0, 0]),
                    "sparse_nz_max": eq(5001)}))
    # three strikes: blocks no pool completes, in a row; after the third give-up the rest runs general.  Probed (blocks 1..3: each is
    # the first block of its pool size) and pipelined (block 1 passes its probe; 2..4 are found after everything was submitted)
    C.append(_case("strikes_probed", 2304, 71, lambda b, r: deficient_block(r) if b in (1, 2, 3) else easy_block(r),
                   {"sparse_blocks": eq([0, 0, 0]), "sparse_panels_first64": eq(0), "sparse_panels_absorb": eq(0), "sparse_panels_rounds": eq(0),
                    "sparse_giveups": eq(3), "sparse_giveup_why": eq([0, 0, 3, 0, 0])}))
    C.append(_case("strikes_pipelined", 2304, 72, lambda b, r: deficient_block(r) if b in (2, 3, 4) else easy_block(r),
                   {"sparse_blocks": eq([1, 0, 0]), "sparse_panels_first64": eq(4), "sparse_panels_absorb": eq(0), "sparse_panels_rounds": eq(0),
                    "sparse_giveups": eq(3), "sparse_giveup_why": eq([0, 0, 3, 0, 0])}))
    # reason 5: a panel with 40 rows that carry a bit in it; reason 2: a block of 240 rows.  Two give-ups: the largest pool behind them
    C.append(_case("reasons_5_and_2", 2304, 81, lambda b, r: short_panel_block(r) if b == 1 else thin_block(r) if b == 2 else easy_block(r),
                   {"sparse_blocks": eq([0, 0, 6]), "sparse_panels_first64": eq(24), "sparse_panels_absorb": eq(0), "sparse_panels_rounds": eq(0),
                    "sparse_giveups": eq(2), "sparse_giveup_why": eq([0, 1, 0, 0, 1])}))
    # alive bound (a): block 9's only rows at the very top -- a zero window for eight blocks; min_zero must hold the bound
    C.append(_case("alive_top", 3072, 91, lambda b, r: easy_block(r, extra=0) if b == 9 else easy_block(r),
                   {"sparse_blocks": eq([11, 0, 0]), "sparse_panels_first64": eq(44), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), **NO_GIVEUP}, order=[9, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11]))
    # (b) home blocks in reverse row order
    C.append(_case("alive_reverse", 2304, 92, lambda b, r: easy_block(r),
                   {"sparse_blocks": eq([8, 0, 0]), "sparse_panels_first64": eq(32), "sparse_panels_absorb": eq(0),
                    "sparse_panels_rounds": eq(0), **NO_GIVEUP}, order=[8, 7, 6, 5, 4, 3, 2, 1]))
    # (c) a pool row that is never taken right behind the first one that is (min_free = 1), which is also (d): the bound is 1, not a
    # multiple of 64, when block 2 starts
    C.append(_case("alive_min_free", 2304, 93, lambda b, r: dup_front_block(r),
                   {"sparse_blocks": eq([8, 0, 0]), "sparse_panels_first64": eq(0), "sparse_panels_absorb": eq(32),
                    "sparse_panels_rounds": eq(0), **NO_GIVEUP}))
    # (c) with teeth: in a diagonal system an untaken pool row is reduced to zero inside its own block, so a bound that skipped it
    # would lose nothing.  Here row 1 is a copy of row 0 within block 1's window AND carries the only bit of column 7 of block 5's
    # panel 2: block 1 leaves it untaken (min_free = 1, no zero-window row above it), and block 5 needs it alive
    C.append(_two_block_row_case())
    # beyond the mask window: 66000 zero rows between the alive bound and block 8's only pivots.  The kernel cannot see them (reason 2)
    C.append(_case("beyond_window", 2304, 95, lambda b, r: easy_block(r),
                   {"sparse_blocks": eq([7, 0, 0]), "sparse_panels_first64": eq(28), "sparse_panels_absorb": eq(0), "sparse_panels_rounds": eq(0),
                    "sparse_giveups": eq(1), "sparse_giveup_why": eq([0, 1, 0, 0, 0]), "sparse_nz_max": eq(320)},
                   layout=lambda blocks: [("block", b) for b in (1, 2, 3, 4, 5, 6, 7, 0)] + [("zero", 66000), ("block", 8)]))
    # inconsistent: the first64 system's kind with three redundant rows' constants flipped (the constants are in no block's window)
    C.append(_case("inconsistent", 2304, 96, lambda b, r: absorb_block(r, 3, 200) if b == 3 else easy_block(r),
                   {"sparse_blocks": ge([8, 0, 0]), "sparse_panels_first64": ge(31), "sparse_panels_absorb": ge(1), "sparse_giveups": ge(0)},
                   consistent=False))
    C.append(_shuffled("shuffled_fill_in_light", 97, 3, 600))
    C.append(_shuffled("shuffled_fill_in_heavy", 98, 12, 2500))
    return C


_CASES = None


def cases() -> dict:
    """name -> Case, built once"""
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in all_cases()}
    return _CASES


NAMES = ["first64", "absorb_100", "absorb_511", "absorb_512", "cycle", "truncated", "escalate_middle", "escalate_largest",
         "straight_to_largest", "escalate_skip_middle", "pipelined", "pipelined_deep", "strikes_probed", "strikes_pipelined", "reasons_5_and_2", "alive_top", "alive_reverse",
         "alive_min_free", "alive_min_free_row_in_two_blocks", "beyond_window", "inconsistent", "shuffled_fill_in_light", "shuffled_fill_in_heavy"]


def holds(stats: dict, expect: dict) -> list:
    """the expectations that `stats` misses, as text (empty: all hold)"""
    bad = []
    for key, (op, want) in expect.items():
        got = sum(stats["sparse_blocks"]) if key == "sparse_blocks_sum" else stats[key]
        if op == "==":
            ok = got == want
        elif isinstance(want, list):
            ok = all(g >= w for g, w in zip(got, want))
        else:
            ok = got >= want
        if not ok:
            bad.append(f"{key}: got {got}, want {op} {want}")
    return bad
