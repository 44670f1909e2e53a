"""Built systems for the one-launch dense block search (block_fast_body: k_block_fast_narrow, k_block_fast + k_narrow_all, k_block_fast
with the general steps behind it) and what each must trigger (inputs and an integer model only -- no solver here).

Premise.  The coefficient support of every row lies inside ONE block (256 consecutive columns = 4 window words); the constant is free.
Eliminating another block never changes such a row and the look-ahead applies zero multipliers to it, so the window the search meets at
block b is exactly what was written for b, in row order.  Its candidates are the first 320 alive rows from the alive bound, whatever
their window holds: all-zero rows and the next block's home rows (zero in this window) are candidates too.  Chunk g (candidates 64g ..
64g + 63) is panel g's main chunk, chunk g + 1 its only completion chunk; chunk 4 serves panel 3 only.

Every block's home rows are exactly 256 independent rows (255 + a dependent one in the three `giveup_panel*` cases), which all die
whoever eliminates the block; every extra row is an all-zero row, which never dies.  So the rows that are alive when a block starts do
not depend on what the general path picked, and `simulate` -- compaction, density gate, gj_columns, column-slot find_absorb, the narrow
step of the unused candidates, new_first, iterated over the blocks with the host's rules of forward_block / block_way --
arrives at gf2bv_stats::fast_blocks.  Where the general path's `fast_off` verdict (k_panel_step's publish: an easy, full last panel)
cannot be read off the construction, the model runs both ways; the count is `("==", v)` where both agree and `(">=", low)` otherwise.

`build_block` writes a block in the order the search will read it, running the model's own panel step as it goes: a word that an
earlier panel's narrow step will have changed by the time it is looked at is written so that it has the designed value THEN.

tests/test_dense_cases_cpu.py proves every case's claim under `simulate` and checks the model's pivot sets against an independent
rank computation; tests/test_gpu_dense_search.py runs the cases."""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

from tests.sparse_cases import DENSE_BITS, DENSE_WORDS, FAST_NC, G, MIN_BLOCKS, eq, ge, holds, rank_of  # noqa: F401  (holds: for the tests)

FEW_MISSING = 8                 # GF2_FEW_MISSING: columns a main chunk may leave to the targeted completion
REACH = 8 * 256                 # block_fast_body: the compaction looks at 8 rounds x 256 rows from the alive bound
FAST_ONLY_ROWS = FAST_NC + 128  # block_way: the dense search alone wants `rows - 256 blk >= 448`
FEW_UNITS = 8                   # GF2_FEW_UNITS: search units of an easy general panel; unit 0's slice starts at the alive bound
HARD_CHUNKS = 8                 # search_panel: a publisher that scanned more than 8 chunks of 64 rows calls the panel hard
GAP = "gap"                     # build_block: a candidate slot that belongs to whatever follows the block (zero in its window)


def bits(x: int):
    while x:
        low = x & -x
        yield low.bit_length() - 1
        x ^= low


def popcount(x: int) -> int:
    return bin(x).count("1")


# ---- the search's arithmetic on plain integers -----------------------------------------------------------------------------------

def gj_columns(words: list, base: int):
    """64 candidate words (0: no candidate) -> (basis, lane_of).  Columns ascending, the first unused candidate that has the bit
    becomes the column's pivot, every other candidate that has the bit takes it (full Gauss-Jordan).  basis: column -> [reduced
    word, combination as a mask over candidate indices `base + lane`]; lane_of: column -> lane of its source."""
    cur = list(words)
    comb = [1 << (base + i) for i in range(64)]
    took, lane_of = 0, {}
    for b in range(64):
        L = next((i for i in range(64) if not (took >> i) & 1 and (cur[i] >> b) & 1), -1)
        if L < 0:
            continue
        took |= 1 << L
        lane_of[b] = L
        v, c = cur[L], comb[L]
        for i in range(64):
            if i != L and (cur[i] >> b) & 1:
                cur[i] ^= v
                comb[i] ^= c
    return {b: [cur[L], comb[L]] for b, L in lane_of.items()}, lane_of


def reduce_by(basis: dict, w: int):
    """w reduced by a fully reduced basis, and the combination that did it"""
    v, c = w, 0
    for p in bits(w):
        if p in basis:
            v ^= basis[p][0]
            c ^= basis[p][1]
    return v, c


def absorb(basis: dict, cands: list) -> list:
    """column-slot find_absorb: the columns without a pivot, ascending; for each the first candidate (cands: [(index, raw word)], in
    lane order) whose REDUCED word has the bit becomes its pivot, and the basis is reduced by it.  -> [(column, index)] taken"""
    taken = []
    for b in [q for q in range(64) if q not in basis]:
        for idx, w in cands:
            if not w:
                continue
            v, c = reduce_by(basis, w)
            if (v >> b) & 1:
                c ^= 1 << idx
                for vc in basis.values():
                    if (vc[0] >> b) & 1:
                        vc[0] ^= v
                        vc[1] ^= c
                basis[b] = [v, c]
                taken.append((b, idx))
                break
    return taken


def panel_step(cw: list, used: list, g: int, completion: list, few, gate: bool) -> dict:
    """One panel of the search on the candidates' window words `cw` ([4 words] each) and `used`, both changed in place.  `completion`:
    the candidate indices the completion may take from.  -> what happened; "why" is None when the panel is complete."""
    base = 64 * g
    main = [0 if used[base + i] else cw[base + i][g] for i in range(64)]
    rec = {"g": g, "main": main, "dense": sum(1 for w in main if popcount(w) > DENSE_BITS), "why": None, "absorbed": [], "next": []}
    if gate and rec["dense"] < DENSE_WORDS:
        rec["why"] = "gate"
        return rec
    basis, lane_of = gj_columns(main, base)
    for L in lane_of.values():
        used[base + L] = True
    src = {b: base + L for b, L in lane_of.items()}
    rec["main_pivots"] = sorted(basis)
    if few is not None and len(basis) < 64 - few:
        rec["why"] = "few"
        return rec
    if len(basis) < 64:
        cands = [(i, 0 if used[i] else cw[i][g]) for i in completion]
        rec["next"] = [w for _, w in cands]
        rec["absorbed"] = absorb(basis, cands)
        for b, i in rec["absorbed"]:
            used[i] = True
            src[b] = i
        if len(basis) < 64:
            rec["why"] = "incomplete"
            return rec
    # the pivot rows' words right of the panel = combination x source words; a source's multipliers of the earlier panels
    P = {b: [0] * G for b in basis}
    for b, (_, c) in basis.items():
        for s in bits(c):
            for e in range(g + 1, G):
                P[b][e] ^= cw[s][e]
    rec["src"] = src
    rec["comb"] = {b: vc[1] for b, vc in basis.items()}
    rec["src_mult"] = {b: tuple(cw[src[b]][:g]) for b in basis}
    rec["pivot_rows"] = P
    rec["narrowed"] = 0
    if g + 1 < G:       # the narrow step of the unused candidates: word g stays (the multiplier), the words right of it change
        for c in range(len(cw)):
            if not used[c] and cw[c][g]:
                rec["narrowed"] += 1
                for b in bits(cw[c][g]):
                    for e in range(g + 1, G):
                        cw[c][e] ^= P[b][e]
    return rec


# ---- one block search, and the blocks of a system under the host's rules ---------------------------------------------------------

def simulate_block(rows: list, dead: list, first: int, b: int) -> dict:
    """block_fast_body on block b: rows = [None | (block, (w0, w1, w2, w3))], dead = who has died, first = the alive bound"""
    n = len(rows)
    rec = {"block": b, "first": first, "taken": False, "why": None, "panels": []}
    if n - first < FAST_NC:
        rec["why"] = "rows"
        return rec
    cand = [i for i in range(first, min(n, first + REACH)) if not dead[i]][:FAST_NC]
    rec["candidates"] = cand
    if len(cand) < FAST_NC:
        rec["why"] = "reach"
        return rec
    assert all(rows[i] is None or rows[i][0] >= b for i in cand), "a home row of an earlier block is still alive"
    cw = [list(rows[i][1]) if rows[i] is not None and rows[i][0] == b else [0] * G for i in cand]
    used = [False] * FAST_NC
    for g in range(G):
        p = panel_step(cw, used, g, list(range(64 * g + 64, 64 * g + 128)), FEW_MISSING, True)
        rec["panels"].append(p)
        if p["why"]:
            rec["why"] = f"{p['why']} {g}"
            return rec
    rec["taken"] = True
    rec["used"] = [cand[c] for c in range(FAST_NC) if used[c]]
    rec["new_first"] = cand[next(c for c in range(FAST_NC) if not used[c])]
    return rec


def general_block(rows: list, dead: list, first: int, b: int) -> dict:
    """The general panel steps on block b: its alive home rows die.  fast_off: 0 where every panel is complete inside what unit 0
    scans in at most 8 chunks from the bound (easy, full last panel), None where that cannot be said from the construction."""
    n = len(rows)
    home = [i for i in range(n) if rows[i] is not None and rows[i][0] == b and not dead[i]]
    vec = {i: sum(w << (64 * e) for e, w in enumerate(rows[i][1])) for i in home}
    rank = rank_of(vec.values())
    units = min(256, max(1, (n + 255) // 256))
    per = (-(-(n - first) // min(units, FEW_UNITS)) + 63) & ~63
    limit = first + min(64 * HARD_CHUNKS, per)
    near = [vec[i] for i in home if i < limit]
    easy = rank == 64 * G and all(rank_of([v & ((1 << (64 * g + 64)) - 1) for v in near]) == 64 * g + 64 for g in range(G))
    for i in home:
        dead[i] = True
    nf = next((i for i in range(first, n) if not dead[i]), n)
    return {"rank": rank, "fast_off": 0 if easy else None, "new_first": nf}


def _run(case, optimistic: bool, unknown_fast_off: int) -> dict:
    rows, n = case.rows, len(case.rows)
    dead, first, fast_off, count, trace = [False] * n, 0, 0, 0, []
    probe = optimistic and case.nblocks >= MIN_BLOCKS and case.full_blocks >= 1 and n >= FAST_NC
    opt = False
    for b in range(case.full_blocks):
        form = "fused" if opt and n - 64 * G * b >= FAST_ONLY_ROWS else "fast+general"
        if fast_off:
            rec = {"block": b, "first": first, "taken": False, "why": "fast_off", "panels": []}
        else:
            rec = simulate_block(rows, dead, first, b)
        rec["form"] = form
        if rec["taken"]:
            for i in rec["used"]:
                dead[i] = True
            first, count, fast_off = rec["new_first"], count + 1, 0
        else:
            if form == "fused":
                opt = False                  # poison: the host resumes at this block with both paths, the rest runs non-optimistic
            gen = general_block(rows, dead, first, b)
            rec["general"] = gen
            first = gen["new_first"]
            fast_off = unknown_fast_off if gen["fast_off"] is None else gen["fast_off"]
            rec["fast_off_after"] = gen["fast_off"]
        if b == 0 and probe:
            opt = rec["taken"]
        trace.append(rec)
    return {"fast_blocks": count, "trace": trace}


def simulate(case, optimistic: bool = True) -> dict:
    """-> fast_blocks as ("==", v) or (">=", low), low / high, and the per-block trace (taken or the reason, rows used, new_first)"""
    hi = _run(case, optimistic, 0)
    unknown = any(r.get("fast_off_after", 0) is None for r in hi["trace"])
    lo = _run(case, optimistic, 1) if unknown else hi
    a, b = sorted((lo["fast_blocks"], hi["fast_blocks"]))
    return {"fast_blocks": eq(a) if a == b else ge(a), "low": a, "high": b, "trace": hi["trace"] if a == b else lo["trace"]}


# ---- writing a block -------------------------------------------------------------------------------------------------------------

def _lane_rng(seed, blk, g, what) -> random.Random:
    return random.Random(f"{seed}/{blk}/{g}/{what}")


def _weighted(rng: random.Random, nbits: int) -> int:
    return sum(1 << q for q in rng.sample(range(64), nbits))


def design_words(seed, blk, g, n: int, n12: int = 0, last: str = "dense", spread: bool = True) -> list:
    """n independent words for the live lanes of a main chunk, lane by lane from a generator of the lane's own (twins share every lane
    but the one they differ in): dense ones (more than 12 bits), then n12 of exactly 12 bits, then the last lane: "dense", "12", "13",
    or "13-1" = the "13" word without its lowest bit.  n < 64 and `spread`: the 64 - n columns that stay without a pivot are spread
    over the word, and the words carry bits there (functions of lower columns), so that a reduced bit is not a raw bit."""
    k = 64 - n
    miss, fmask = [], {}
    if k and spread and not n12 and last == "dense":
        r = _lane_rng(seed, blk, g, "missing")
        miss = sorted(r.sample(range(8, 64), k))
        for c in miss:
            fmask[c] = r.getrandbits(64) & ((1 << c) - 1) & ~sum(1 << q for q in miss)
    out = []
    for j in range(n):
        kind = last if j == n - 1 else ("12" if j >= n - 1 - n12 else "dense")
        r = _lane_rng(seed, blk, g, f"lane{j}")
        while True:
            if kind == "dense":
                w = r.getrandbits(64)
                for c in miss:
                    w = (w & ~(1 << c)) | ((popcount(w & fmask[c]) & 1) << c)
                ok = popcount(w) > DENSE_BITS + 4
            elif kind == "12":
                w, ok = _weighted(r, DENSE_BITS), True
            else:
                w13 = _weighted(r, DENSE_BITS + 1)
                ok = rank_of(out + [w13 & (w13 - 1)]) == len(out) + 1 and rank_of(out + [w13]) == len(out) + 1
                w = w13 if kind == "13" else w13 & (w13 - 1)
            if ok and rank_of(out + [w]) == len(out) + 1:
                out.append(w)
                break
    return out


def build_block(seed, blk: int, lead: int = 0, zeros=(), comp_lanes=None, far=None, sparse=None, deficient=None,
                copy_rate: float = 0.12) -> dict:
    """The rows of block blk as the search will read them.  Candidates 0 .. lead - 1 are zero rows it inherits (alive rows below its
    own); `zeros`: candidate indices of zero rows of its own; comp_lanes: panel -> lanes of chunk g + 1 that complete it, in COLUMN
    order (default: drawn); far: panel -> candidate index of its one completing row, outside chunk g + 1; sparse: panel -> (n12,
    last) for design_words; deficient: a panel whose last live word is replaced by a combination of two others once the block is
    written (rank 63 over everything).  -> {"list": [(blk, words) | None | GAP] from candidate `lead` on, "role", "comp"}"""
    rng = random.Random(f"{seed}/{blk}/block")
    comp_lanes, far, sparse = dict(comp_lanes or {}), dict(far or {}), dict(sparse or {})
    role = {i: ("lead",) for i in range(lead)}
    role.update({z: ("zero",) for z in zeros})
    role.update({idx: ("comp", q) for q, idx in far.items()})
    comp, live = {}, {}
    for g in range(G):
        live[g] = [64 * g + l for l in range(64) if 64 * g + l not in role]
        for i in live[g]:
            role[i] = ("live", g)
        need = 64 - len(live[g]) - (g in far)
        free = [l for l in range(64) if 64 * g + 64 + l not in role]
        lanes = list(comp_lanes[g]) if g in comp_lanes else rng.sample(free, need)
        assert len(lanes) == need and all(l in free for l in lanes), (g, need, lanes)
        comp[g] = [64 * g + 64 + l for l in lanes] + ([far[g]] if g in far else [])
        for i in comp[g]:
            role[i] = ("comp", g)
    own = sorted(i for i, r in role.items() if r[0] in ("live", "comp"))
    assert len(own) == 64 * G
    top = max(own) + 1
    raw = [[0] * G for _ in range(max(top, FAST_NC))]
    for i in own:
        for e in range(role[i][1] + 1, G):
            raw[i][e] = rng.getrandbits(64)
    cw = [list(w) for w in raw]
    used = [False] * len(cw)
    designed = {}

    def put(i, g, value):               # word g of candidate i is to read `value` when panel g looks at it
        raw[i][g] = value ^ cw[i][g]
        cw[i][g] = value

    for g in range(G):
        D = design_words(seed, blk, g, len(live[g]), *sparse.get(g, (0, "dense")))
        for i, d in zip(live[g], D):
            put(i, g, d)
            designed[i] = d
        missing = sorted(set(range(64)) - set(gj_columns([cw[64 * g + l][g] if 64 * g + l in live[g] else 0 for l in range(64)], 64 * g)[0]))
        assert len(missing) == len(comp[g])
        span = D[:-1]                   # (the last live word stays out of every combination: `deficient` replaces it)
        for j, i in enumerate(comp[g]):
            pattern = (1 << missing[j]) | sum(1 << c for c in missing[j + 1:] if rng.random() < 0.5)
            while True:                 # (the first one is taken although its RAW word lacks the column's bit)
                word = pattern
                for v in rng.sample(span, min(len(span), 5)):
                    word ^= v
                if j or not (word >> missing[0]) & 1:
                    break
            put(i, g, word)
        for i in own:
            if not used[i] and role[i][1] > g:          # rows of later panels: zero, or a combination of this panel's rows
                c = 0
                if rng.random() < copy_rate:
                    for v in rng.sample(span, 3):
                        c ^= v
                put(i, g, c)
        p = panel_step(cw, used, g, sorted(comp[g]), None, False)
        assert p["why"] is None and [i for _, i in p["absorbed"]] == comp[g], "the block is not what its plan says"
    if deficient is not None:
        a, b, c = live[deficient][0], live[deficient][1], live[deficient][-1]
        raw[c][deficient] ^= designed[c] ^ designed[a] ^ designed[b]
    out = []
    for i in range(lead, top):
        kind = role.get(i, ("foreign",))[0]
        out.append(None if kind == "zero" else GAP if kind == "foreign" else (blk, tuple(raw[i])))
    return {"list": out, "role": role, "comp": comp, "live": live}


# ---- a system ----------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    cols: int
    rows: list                     # None (a zero row) | (block, (w0, w1, w2, w3))
    expect: dict                   # {"fast_blocks": (op, value)}
    claim: object                  # trace -> None: asserts what the case is named for
    block: int = -1                # the block the case is about
    env: dict = field(default_factory=dict)
    deficit: int = 0               # cols - rank
    plans: dict = field(default_factory=dict, repr=False)     # block -> build_block's result
    seed: int = 0
    note: str = ""
    _built: dict = field(default_factory=dict, repr=False)

    @property
    def full_blocks(self) -> int:
        return self.cols // (64 * G)

    @property
    def nblocks(self) -> int:
        return -(-((self.cols + 1 + 63) // 64) // G)

    def aug(self) -> np.ndarray:
        """the packed augmented matrix (rows x words, column `cols` = constant), constants from a planted solution"""
        if "aug" not in self._built:
            wt = (self.cols + 1 + 63) // 64
            rng = random.Random(self.seed ^ 0x5EED)
            plant = [rng.getrandbits(64) for _ in range(wt)]
            a = np.zeros((len(self.rows), wt), dtype=np.uint64)
            const = np.zeros(len(self.rows), dtype=np.uint64)
            for i, r in enumerate(self.rows):
                if r is None:
                    continue
                for e, w in enumerate(r[1]):
                    a[i, G * r[0] + e] = w
                    const[i] ^= popcount(w & plant[G * r[0] + e]) & 1
            a[:, self.cols // 64] |= const << np.uint64(self.cols % 64)
            self._built["aug"] = a
        return self._built["aug"]

    def model(self, optimistic: bool = True) -> dict:
        if optimistic not in self._built:
            self._built[optimistic] = simulate(self, optimistic)
        return self._built[optimistic]


_PLAIN = {}


def _plain_block(b: int) -> dict:
    """the block every case uses where it has nothing to say: built once"""
    if b not in _PLAIN:
        _PLAIN[b] = build_block("plain", b)
    return _PLAIN[b]


def _system(name, nb, seed, specs, tail, expect, claim, block=-1, top_zero=0, **kw) -> Case:
    """nb full blocks written by build_block(**specs[b]), each block's gaps filled from what follows it, `tail` zero rows behind"""
    plans = {b: build_block(seed, b, **specs[b]) if b in specs else _plain_block(b) for b in range(nb)}
    stream = [None] * tail
    for b in reversed(range(nb)):
        out = [stream.pop(0) if e is GAP else e for e in plans[b]["list"]]
        stream = out + stream
    return Case(name, 64 * G * nb, [None] * top_zero + stream, {"fast_blocks": expect}, claim, block=block, plans=plans, seed=seed, **kw)


NB = 10                          # 2560 columns: 10 full blocks and the constant's block
LATE = NB - 2                    # a case block whose count is exact: no zero tail, so the last full block has fewer than 320 rows left
TAIL = 512                       # zero rows behind the last block where every block is to stay eligible


def _taken(t, blocks, but=()):
    assert [r["block"] for r in t if r["taken"]] == [b for b in blocks if b not in but], [(r["block"], r["why"]) for r in t]


def _late(name, seed, spec, expect_taken: bool, claim, **kw) -> Case:
    """plain blocks, the case block as block LATE, one plain block behind it that no search can reach"""
    def whole(t):
        _taken(t, range(LATE + 1), () if expect_taken else (LATE,))
        assert t[LATE + 1]["why"] in ("rows", "reach", "fast_off")
        assert t[LATE]["form"] == "fused" and t[LATE + 1]["form"] == "fast+general"
        claim(t[LATE])
    return _system(name, NB, seed, {LATE: spec}, 0, eq(LATE + 1 if expect_taken else LATE), whole, block=LATE, **kw)


def _absorbed(rec, g):
    return [i - 64 * (g + 1) for _, i in rec["panels"][g]["absorbed"]]


K8_LANES = [31, 0, 47, 63, 5, 58, 12, 22]       # completing lanes of a miss_8 panel in column order: 0, 63 and six in between, out of order


def _miss_case(k: int, g: int) -> Case:
    # (miss_9 shares the seed and eight of its nine zero lanes with miss_8)
    lanes = random.Random(f"miss/{min(k, 8)}/{g}").sample(range(64), min(k, 8))
    if k == 9:
        lanes.append(next(l for l in range(64) if l not in lanes))
    spec = {"zeros": sorted(64 * g + l for l in lanes)}
    if k >= 8:
        spec["comp_lanes"] = {g: K8_LANES + ([40] if k == 9 else [])}

    def claim(r):
        p = r["panels"][g]
        assert sum(1 for w in p["main"] if w == 0) == k and len(p["main_pivots"]) == 64 - k
        if k <= FEW_MISSING:
            assert r["taken"] and len(p["absorbed"]) == k and [c for c, _ in p["absorbed"]] == sorted(c for c, _ in p["absorbed"])
            for q in range(g + 1, G):       # the chain behind it: the rows it absorbed are `used` in the next main chunk
                assert len(r["panels"][q]["absorbed"]) == k and sum(1 for w in r["panels"][q]["main"] if w == 0) == k
            if k == 8:
                assert _absorbed(r, g) == K8_LANES
            c, i = p["absorbed"][0]         # a reduced bit is not the raw bit: the first row is taken for a column its raw word lacks
            assert not (p["next"][i - 64 * (g + 1)] >> c) & 1
        else:
            assert not r["taken"] and r["why"] == f"few {g}"
    return _late(f"miss_{k}_g{g}", 1000 + 8 * g, spec, k <= FEW_MISSING, claim)


def _absorb_twin(g: int, last_lane: bool) -> Case:
    spec = {"zeros": [64 * g + 20]}
    if last_lane:
        spec["comp_lanes"] = {g: [63]}
    else:
        spec["far"] = {g: 64 * (g + 2)}

    def claim(r):
        p = r["panels"][g]
        assert len(p["main_pivots"]) == 63
        if last_lane:
            assert r["taken"] and _absorbed(r, g) == [63]
        else:
            assert r["why"] == f"incomplete {g}" and rank_of(p["main"] + p["next"]) == 63
    return _late(f"absorb_{'last_lane' if last_lane else 'incomplete'}_g{g}", 2000 + g, spec, last_lane, claim)


def _chain_case() -> Case:
    zeros = [5, 40, 64 + 9, 128 + 3, 128 + 50]

    def claim(r):
        assert r["taken"] and [len(p["absorbed"]) for p in r["panels"]] == [2, 3, 5, 5]
        for g in range(1, G):
            p = r["panels"][g]
            # sources that were candidates of an earlier panel's narrow step carry multipliers for it
            assert any(any(m) for m in p["src_mult"].values())
            assert r["panels"][g - 1]["narrowed"] > 0
        assert any(m[0] and m[1] for b, m in r["panels"][2]["src_mult"].items() if r["panels"][2]["src"][b] >= 192)
    return _late("chain", 3000, {"zeros": zeros, "copy_rate": 0.3}, True, claim)


def _dense_case(name, g, n12, last, want_dense, zeros=()) -> Case:
    def claim(r):
        p = r["panels"][g]
        assert p["dense"] == want_dense and sum(1 for w in p["main"] if w == 0) == len(zeros)
        assert all(popcount(w) == DENSE_BITS for w in p["main"] if w and popcount(w) <= DENSE_BITS)
        assert rank_of(p["main"]) == 64 - len(zeros)
        if want_dense >= DENSE_WORDS:
            assert r["taken"]
        else:
            assert r["why"] == f"gate {g}"
    return _late(name, 4000 + g, {"sparse": {g: (n12, last)}, "zeros": list(zeros)}, want_dense >= DENSE_WORDS, claim)


def _giveup_case(g: int) -> Case:
    def claim(r):
        p = r["panels"][g]
        assert r["why"] == f"incomplete {g}" and len(p["main_pivots"]) == 63 and rank_of(p["main"] + p["next"]) == 63
        assert len(r["panels"]) == g + 1 and all(q["why"] is None for q in r["panels"][:g])      # panels 0 .. g - 1 were published
        assert r["general"]["rank"] == 64 * G - 1
    return _late(f"giveup_panel{g}", 5000 + g, {"deficient": g}, False, claim, deficit=1)


def _anchored(name, seed, j, c, expect, claim, nb=NB) -> Case:
    """block j has a zero row of its own as candidate c: the bound stops there, and every block behind it starts with that row"""
    specs = {b: {"lead": 1} for b in range(j + 1, nb)}
    specs[j] = {"zeros": [c]}
    return _system(name, nb, seed, specs, TAIL, expect, claim, block=j)


def all_cases() -> list:
    C = []

    def plain_claim(t):
        _taken(t, range(NB))
        assert all(not p["absorbed"] and len(p["main_pivots"]) == 64 for r in t for p in r["panels"])
        assert [r["new_first"] for r in t] == [256 * (b + 1) for b in range(NB)]
        assert all(r["form"] == "fused" for r in t[1:]) and t[0]["form"] == "fast+general"
    C.append(_system("plain", NB, 100, {}, TAIL, eq(NB), plain_claim))
    for k in (1, 2, 4, 7, 8):
        for g in range(G):
            C.append(_miss_case(k, g))
    for g in range(G):
        C.append(_miss_case(9, g))
    for g in (0, 2):
        C.append(_absorb_twin(g, False))
        C.append(_absorb_twin(g, True))
    C.append(_chain_case())
    C.append(_dense_case("dense_48", 0, 16, "dense", 48))
    C.append(_dense_case("dense_47", 0, 16, "12", 47))
    C.append(_dense_case("dense_13", 2, 16, "13", 48))
    C.append(_dense_case("dense_12", 2, 16, "13-1", 47))
    carry = [3, 9, 17, 26, 33, 41, 50, 60]         # eight zero rows in chunk 0: panel 0 absorbs eight rows of chunk 1, `used` in panel 1
    C.append(_dense_case("dense_carry_48", 1, 8, "dense", 48, carry))
    C.append(_dense_case("dense_carry_47", 1, 8, "12", 47, carry))
    for g in (0, 2, 3):
        C.append(_giveup_case(g))

    def back_claim(t):
        _taken(t, range(NB), (3,))
        assert t[3]["why"] == "gate 1" and t[3]["form"] == "fused" and t[3]["general"]["fast_off"] == 0 and t[3]["general"]["rank"] == 256
        assert t[4]["form"] == "fast+general" and t[4]["first"] == 1024
    C.append(_system("giveup_then_back", NB, 6000, {3: {"sparse": {1: (16, "12")}}}, TAIL, eq(NB - 1), back_claim, block=3))

    def refused_claim(t):
        _taken(t, range(NB), (0,))
        assert t[0]["why"] == "gate 0" and t[0]["general"]["fast_off"] == 0 and all(r["form"] == "fast+general" for r in t)
    C.append(_system("first_block_refused", NB, 6100, {0: {"sparse": {0: (16, "12")}}}, TAIL, eq(NB - 1), refused_claim, block=0,
                     env={"GF2BV_SPARSE_FAST": "0"}))

    def anchor_claim(t):
        _taken(t, range(7))
        assert all(r["first"] == 0 for r in t) and all(r["why"] == "reach" or r["why"] == "fast_off" for r in t[7:]) and t[7]["why"] == "reach"
        assert all(r["candidates"][0] == 0 and [len(p["absorbed"]) for p in r["panels"]] == [1] * G for r in t[:7])
    C.append(_system("anchor_zero_row", NB, 6200, {b: {"lead": 1} for b in range(NB)}, TAIL, eq(7), anchor_claim, block=7, top_zero=1))

    def edge_claim(offset):
        def claim(t):
            bound = t[2]["first"]
            assert all(r["first"] == bound for r in t[2:])
            full = [i for i in range(bound, bound + 4096) if i not in dead_before(t, 8)][:FAST_NC]
            assert full[-1] - bound == offset
            _taken(t, range(9 if offset < REACH else 8))
            assert t[9]["why"] in ("reach", "fast_off") and (offset < REACH or t[8]["why"] == "reach")
        return claim
    C.append(_anchored("anchor_edge_2047", 6300, 1, 64, eq(9), edge_claim(2047)))
    C.append(_anchored("anchor_edge_2048", 6300, 1, 63, eq(8), edge_claim(2048)))

    def tail_claim(left):
        def claim(t):
            _taken(t, range(NB if left >= FAST_NC else NB - 1))
            assert t[9]["first"] == 2304 and t[9]["form"] == "fast+general" and t[8]["form"] == "fused"      # 448-row rule: 576 and 320 rows left
            assert left >= FAST_NC or t[9]["why"] == "rows"
        return claim
    C.append(_system("tail_320", NB, 6400, {}, 64, eq(NB), tail_claim(320), block=9))
    C.append(_system("tail_319", NB, 6400, {}, 63, eq(NB - 1), tail_claim(319), block=9))

    def leftover_claim(c):
        def claim(t):
            _taken(t, range(NB))
            assert t[3]["new_first"] == 768 + c and all(r["first"] == 768 + c and r["candidates"][0] == 768 + c for r in t[4:])
        return claim
    C.append(_anchored("leftover_low", 6500, 3, 0, eq(NB), leftover_claim(0)))
    C.append(_anchored("leftover_mid", 6501, 3, 70, eq(NB), leftover_claim(70)))

    def seven_claim(t):
        _taken(t, range(6))
        assert all(r["form"] == "fast+general" for r in t)
    C.append(_system("seven_blocks", 6, 6600, {}, TAIL, eq(6), seven_claim))
    return C


def dead_before(trace, b) -> set:
    """rows that blocks before b used (taken blocks only)"""
    return {i for r in trace[:b] if r["taken"] for i in r["used"]}


NAMES = (["plain"] + [f"miss_{k}_g{g}" for k in (1, 2, 4, 7, 8) for g in range(G)] + [f"miss_9_g{g}" for g in range(G)]
         + ["absorb_incomplete_g0", "absorb_last_lane_g0", "absorb_incomplete_g2", "absorb_last_lane_g2", "chain",
            "dense_48", "dense_47", "dense_13", "dense_12", "dense_carry_48", "dense_carry_47",
            "giveup_panel0", "giveup_panel2", "giveup_panel3", "giveup_then_back", "first_block_refused",
            "anchor_zero_row", "anchor_edge_2047", "anchor_edge_2048", "tail_320", "tail_319", "leftover_low", "leftover_mid", "seven_blocks"])

# twins: (the one that is taken, the one that gives up, the block they differ in)
TWINS = ([(f"miss_8_g{g}", f"miss_9_g{g}") for g in range(G)]
         + [("absorb_last_lane_g0", "absorb_incomplete_g0"), ("absorb_last_lane_g2", "absorb_incomplete_g2"),
            ("dense_48", "dense_47"), ("dense_13", "dense_12"), ("dense_carry_48", "dense_carry_47"),
            ("anchor_edge_2047", "anchor_edge_2048"), ("tail_320", "tail_319")])

_CASES = None


def cases() -> dict:
    """name -> Case, built once"""
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in all_cases()}
    return _CASES
