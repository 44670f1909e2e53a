"""Built systems for the general panel search (search_panel and the narrow half of k_panel_step) and what each must trigger (inputs
and an integer model only -- no solver here).

Premise (the one of tests/sparse_cases.py).  The coefficient support of every row lies inside ONE 64-column panel; the constant is free.
Eliminating another panel never changes such a row and causes no fill-in, so the candidates panel j meets are the rows written for j,
in place, and every other alive row is a candidate whose word is zero.  A row dies only as a source of its own panel.

Model.  `simulate` follows the host and the kernel as written: units = min(256, ceil(rows / 256)); per panel `active` (8 units, or all
when the panel before was hard), the slices of `per` rows (rounded up to 64) from the alive bound, each unit's scan in 64-row chunks
that stops at a full basis -- the first chunk through gj_columns when 48 of its 64 words have more than 12 bits (not on a wide panel,
not on a panel of fewer than 64 columns), kept at 56 pivots and redone row-wise below that -- then the arrival: unit 0's record if it is
complete, else the first complete one, else the merge of the lists packed into chunks of 64 with a carry; group by group (16 units) on
a wide panel of more than 16 units; `hard`, `wide`, and the new bound by both routes.  The pivot choice is the kernel's in every path
(columns ascending, the first candidate of the chunk whose reduced word has the bit: dense_cases.absorb), so the sources, the order of
every list and with them the bound are exact.  The model's switches (`few_units`, `group`, `carry`, `exclude_sources`) are the four
mutants of profiles/general_search_mutants.txt: tests/test_general_cases_cpu.py shows that each of them moves a prediction.

Every count in the table is exact (`("==", v)`): gf2bv_stats::general_*.  What no counter tells apart -- the targeted path of
find_absorb, the carry, a merge that stops before its last list, empty lists, the route of the bound -- is in the model's per-panel
trace, which the CPU test reads for each case's claim, and reaches the GPU through the answers (rank and pivots need every source)."""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

from tests import dense_cases as DC
from tests.sparse_cases import DENSE_BITS, DENSE_WORDS, G, M64, copies, eq, holds, independent_words, rank_of  # noqa: F401

FEW_UNITS = DC.FEW_UNITS        # GF2_FEW_UNITS
FEW_MISSING = DC.FEW_MISSING    # GF2_FEW_MISSING
HARD_CHUNKS = DC.HARD_CHUNKS
GROUP = 16                      # GF2_GROUP: units per group of a two-level arrival
MAX_UNITS = 256
NEVER = 0x7F7F7F7F              # GF2_NEVER
MERGED_CHUNKS = 1 << 20         # the `chunks` of a merged group record

COUNTERS = ("general_unit0", "general_adopted", "general_merged", "general_wide", "general_two_level", "general_group_adopted",
            "general_group_merged", "general_gj_kept", "general_gj_redone", "general_chunks")


def units_of(rows: int) -> int:
    return min(MAX_UNITS, max(1, (rows + 255) // 256))


def narrow_rpt(rows: int) -> int:
    """solver_alloc: row blocks of 256 per narrow workgroup (a single system)"""
    return min(8, max(1, ((rows + 255) // 256) // 256))


# ---- the search on plain integers ---------------------------------------------------------------------------------------------------

def _absorb(basis: dict, chunk: list, words: list, mask: int) -> list:
    """one find_absorb step: chunk = 64 rows (-1: none) -> [(column, row)] taken, in the order the slots are handed out"""
    took = DC.absorb(basis, [(lane, (words[r] & mask) if r >= 0 else 0) for lane, r in enumerate(chunk)])
    return [(b, chunk[lane]) for b, lane in took]


def scan_unit(words: list, died: list, j: int, lo: int, hi: int, nrows: int, mask: int, wide: bool) -> dict:
    """search_panel, one unit's slice [lo, hi)"""
    full = DC.popcount(mask)
    basis, order, colslots, gj, chunks, fns, targeted = {}, [], False, None, 0, -1, 0
    base = lo
    while base < hi and len(basis) < full:
        ok = [base + l < hi and died[base + l] >= j for l in range(64)]
        chunk = [base + l if ok[l] else -1 for l in range(64)]
        took = None
        if chunks == 0 and full == 64 and not wide and sum(DC.popcount(words[r] & mask) > DENSE_BITS for r in chunk if r >= 0) >= DENSE_WORDS:
            b2 = {}
            t2 = _absorb(b2, chunk, words, mask)
            if len(b2) >= 64 - FEW_MISSING:
                basis, colslots, gj, took = b2, True, "kept", t2
            else:
                gj = "redone"
        if took is None:
            targeted += bool(basis) and full - len(basis) <= FEW_MISSING
            took = _absorb(basis, chunk, words, mask)
        order += took
        chunks += 1
        if fns < 0:
            taken = {r for _, r in took}
            fns = next((r for r in chunk if r >= 0 and r not in taken), -1)
        base += 64
    if fns < 0:
        fns = min(base, nrows)
    srow = [r for _, r in (sorted(order) if colslots else order)]          # column slots: packed by column
    return {"cnt": len(basis), "srow": srow, "chunks": chunks, "first_nonsrc": fns, "gj": gj, "targeted": targeted,
            "stopped_early": len(basis) == full and base < hi}


def merge_lists(lists: list, words: list, mask: int, carry: bool = True) -> dict:
    """search_panel's merge_lists over source-row lists: packed into chunks of 64, stops at a full basis"""
    full = DC.popcount(mask)
    basis, order, pend = {}, [], []
    info = {"read": 0, "empty": 0, "carried": 0, "sum": 0, "targeted": 0}

    def absorb_rows(chunk):
        info["targeted"] += bool(basis) and full - len(basis) <= FEW_MISSING
        order.extend(_absorb(basis, chunk + [-1] * (64 - len(chunk)), words, mask))

    for lst in lists:
        if len(basis) >= full:
            break
        info["read"] += 1
        if not lst:
            info["empty"] += 1
            continue
        info["sum"] += len(lst)
        pend += lst
        if len(pend) >= 64:
            absorb_rows(pend[:64])
            rest = pend[64:]
            info["carried"] += len(rest)
            pend = rest if carry else pend[:len(rest)]         # (the mutant: the staging keeps its head)
    if pend and len(basis) < full:
        absorb_rows(pend)
    info.update(cnt=len(basis), srow=[r for _, r in order], lists=len(lists))
    return info


def simulate(case, few_units: int = FEW_UNITS, group: int = GROUP, carry: bool = True, exclude_sources: bool = True, fast: bool = False,
             heed_fast_off: bool = True) -> dict:
    """every panel of `case` through search_panel: gf2bv_stats::general_* and, per panel, what happened ("trace").
    fast: as shipped where the host enqueues k_block_fast with the general steps behind it for every full block (every case here: fewer
    than 8 blocks, so neither the optimistic enqueue nor the sparse search is tried; a gang) -- the dense search (dense_cases.
    simulate_block) is asked first unless `fast_off` stands, a block it takes adds 1 to `fast_blocks` and nothing to general_*, and
    `fast_off` is what the block's last general panel leaves: 0 after an easy, full one, else 1 (heed_fast_off=False: a search that
    ignored the flag, for the CPU test's "the flag is what withholds the block")."""
    rows, nrows, cols = case.rows, len(case.rows), case.cols
    units = units_of(nrows)
    st = {k: 0 for k in COUNTERS}
    st.update(trace=[], rank=0, units=units, fast_blocks=0, blocks=[])
    died = [NEVER] * nrows
    first, wide, fast_off, taken_until = 0, False, 0, 0
    npanels = (cols + 63) // 64
    for j in range(npanels):
        if fast and j % G == 0 and (j + G) * 64 <= cols and nrows >= DC.FAST_NC:
            blk = {"block": j // G, "first": first, "fast_off_before": fast_off, "taken": False}
            if not (fast_off and heed_fast_off):
                view = [(r[0] // G, tuple(r[1] if r[0] % G == e else 0 for e in range(G))) if r is not None and r[0] // G == j // G else None
                        for r in rows]
                rec = DC.simulate_block(view, [d != NEVER for d in died], first, j // G)
                blk["why"] = rec["why"]
                if rec["taken"]:
                    for i in rec["used"]:
                        died[i] = j
                    first, wide, taken_until = rec["new_first"], False, j + G
                    st["fast_blocks"] += 1
                    st["rank"] += 64 * G
                    blk["taken"] = True
            else:
                blk["why"] = "fast_off"
            fast_off = 0 if blk["taken"] else 1
            st["blocks"].append(blk)
        if j < taken_until:
            st["trace"].append({"j": j, "pick": "fast", "p": 64, "srow": None})
            continue
        mask = M64 if cols - 64 * j >= 64 else (1 << (cols - 64 * j)) - 1
        full = DC.popcount(mask)
        words = [r[1] if r is not None and r[0] == j else 0 for r in rows]
        active = units if wide else min(units, few_units)
        n = nrows - first
        per = ((n + active - 1) // active + 63) & ~63 if n > 0 else 0
        U = []
        for u in range(units):
            if u < active:
                lo = first + u * per
                U.append(scan_unit(words, died, j, lo, min(lo + per, nrows), nrows, mask, wide))
            else:
                U.append({"cnt": 0, "srow": [], "chunks": 0, "first_nonsrc": -1, "gj": None, "targeted": 0, "stopped_early": False})
        t = {"j": j, "first": first, "wide": wide, "active": active, "per": per, "full": full, "units": U, "groups": []}
        two_level = wide and units > group
        recs = U[:active]
        if two_level:
            recs = []
            for g0 in range(0, units, group):
                members = U[g0:g0 + group]
                v = next((m for m in members if m["cnt"] == full), None) if full > 0 else None
                if v is not None:
                    recs.append({"cnt": full, "srow": v["srow"], "chunks": v["chunks"], "gj": v["gj"], "how": "adopt", "size": len(members)})
                    st["general_group_adopted"] += 1
                else:
                    m = merge_lists([x["srow"] for x in members], words, mask, carry)
                    recs.append({"cnt": m["cnt"], "srow": m["srow"], "chunks": MERGED_CHUNKS, "gj": None, "how": "merge", "size": len(members), "merge": m})
                    st["general_group_merged"] += 1
            t["groups"] = recs
        pick = None
        if full > 0:
            if U[0]["cnt"] == full:
                pick, t["pick"] = U[0], "unit0"
            else:
                at = next((i for i, r in enumerate(recs) if r["cnt"] == full), -1)
                if at >= 0:
                    pick, t["pick"], t["pick_at"] = recs[at], ("group" if two_level else "unit"), at
        if pick is not None:
            srow, hard = pick["srow"], pick["chunks"] > HARD_CHUNKS
            st["general_chunks"] += pick["chunks"] if pick["chunks"] < MERGED_CHUNKS else 0
            st["general_gj_kept"] += pick["gj"] == "kept"
            st["general_gj_redone"] += pick["gj"] == "redone"
            t["chunks"], t["gj"] = pick["chunks"], pick["gj"]
        else:
            m = merge_lists([r["srow"] for r in recs], words, mask, carry)
            srow, hard = m["srow"], True
            t["pick"], t["merge"] = "merge", m
        st["general_unit0" if pick is U[0] and pick is not None else "general_adopted" if pick is not None else "general_merged"] += 1
        st["general_wide"] += wide
        st["general_two_level"] += two_level
        if pick is U[0] and pick is not None:
            new_first, t["route"] = U[0]["first_nonsrc"], "unit 0"
        else:
            src = set(srow) if exclude_sources else set()
            new_first = next((i for i in range(first, nrows) if died[i] >= j and i not in src), nrows)
            t["route"] = "advance"
        for r in srow:
            died[r] = j
        t.update(p=len(srow), srow=srow, hard=hard, new_first=new_first, two_level=two_level)
        if j % G == G - 1 or j == npanels - 1:                 # the last panel of a block says whether the dense search is worth trying
            fast_off = t["fast_off"] = 0 if not hard and len(srow) == 64 else 1
        st["trace"].append(t)
        st["rank"] += len(srow)
        first, wide = new_first, hard
    return st


# ---- words --------------------------------------------------------------------------------------------------------------------------

def dense(rng, n: int = 64) -> list:
    """n independent words with more than 12 bits each"""
    out = independent_words(rng, n)
    assert all(DC.popcount(w) > DENSE_BITS for w in out)
    return out


def dense_copies(rng, span: list, n: int) -> list:
    out = copies(rng, span, n)
    assert all(DC.popcount(w) > DENSE_BITS for w in out)
    return out


def thin_independent(rng, n: int, beside: list) -> list:
    """n words of 8 bits that are independent of each other and of `beside`"""
    out = []
    while len(out) < n:
        w = 0
        for _ in range(8):
            w |= 1 << rng.randrange(64)
        if rank_of(beside + out + [w]) == len(beside) + len(out) + 1:
            out.append(w)
    return out


def stair(rng, columns, top: int = 64) -> list:
    """one word per column c of `columns`: bit c and random bits above it (below `top`).  Independent, and whatever chunk holds some of
    them, the elimination takes them in this order (distinct lowest bits: no word is changed before its own column comes up)"""
    return [(1 << c) | (rng.getrandbits(64) & ((1 << top) - 1) & ~((2 << c) - 1)) for c in columns]


# ---- a system -----------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    cols: int
    rows: list                     # per row: None (all-zero coefficients) or (panel, word)
    expect: dict                   # counter -> ("==", value)
    claim: object                  # trace -> None, asserting what the case is named for
    note: str = ""
    seed: int = 0
    tall: bool = False
    _built: dict = field(default_factory=dict, repr=False)

    def aug(self) -> np.ndarray:
        """the packed augmented matrix (column `cols` = the constant), constants from a planted solution"""
        if "aug" not in self._built:
            wt = (self.cols + 1 + 63) // 64
            rng = random.Random(self.seed ^ 0x6E4)
            plant = [rng.getrandbits(64) for _ in range(wt)]
            a = np.zeros((len(self.rows), wt), dtype=np.uint64)
            const = np.zeros(len(self.rows), dtype=np.uint64)
            for i, r in enumerate(self.rows):
                if r is not None:
                    a[i, r[0]] = r[1]
                    const[i] = bin(r[1] & plant[r[0]]).count("1") & 1
            a[:, self.cols // 64] |= const << np.uint64(self.cols % 64)
            self._built["aug"] = a
        return self._built["aug"]

    def model(self) -> dict:
        if "model" not in self._built:
            self._built["model"] = simulate(self)
        return self._built["model"]

    def shipped(self) -> dict:
        """the model with the dense block search in front of the general steps"""
        if "shipped" not in self._built:
            self._built["shipped"] = simulate(self, fast=True)
        return self._built["shipped"]

    def panel_rank(self, j: int) -> int:
        return rank_of([r[1] for r in self.rows if r is not None and r[0] == j])

    def rank(self) -> int:
        return sum(self.panel_rank(j) for j in range((self.cols + 63) // 64))


class Sheet:
    """rows being written: put(panel, at, words) places words in consecutive rows"""

    def __init__(self, nrows: int, cols: int):
        self.rows, self.cols = [None] * nrows, cols

    def put(self, panel: int, at: int, words: list) -> None:
        lim = min(64, self.cols - 64 * panel)
        for k, w in enumerate(words):
            assert self.rows[at + k] is None and 0 < w < (1 << lim), (panel, at + k)
            self.rows[at + k] = (panel, w)

    def plain(self, rng, panels, at=None) -> None:
        """64 dense independent rows per panel, panel j at rows 64 j (or from `at` on, one after the other)"""
        for k, j in enumerate(panels):
            self.put(j, 64 * j if at is None else at + 64 * k, dense(rng))


def exact(**kw) -> dict:
    out = {k: eq(0) for k in COUNTERS}
    out.update({"general_" + k: eq(v) for k, v in kw.items()})
    return out


A_ROWS, A_COLS = 2048, 512      # 8 units (every one active, wide or not), 8 panels in two blocks; too large for the one-workgroup path
A_LAST, A_BASE = 7, 448         # the plain panels 0 .. 6 leave the bound at 448: panel 7's unit u scans [448 + 256 u, 704 + 256 u)


def _a(name, seed, write, expect, claim, special=A_LAST, **kw) -> Case:
    rng = random.Random(seed)
    sh = Sheet(A_ROWS, A_COLS)
    sh.plain(rng, range(special))
    write(sh, rng)
    return Case(name, A_COLS, sh.rows, expect, claim, seed=seed, **kw)


def _panel(t, j):
    return t["trace"][j]


def all_cases() -> list:
    C = []

    # every panel: unit 0's first chunk is 64 dense independent rows -- gj_columns keeps all 64, the unit stops after one chunk of its
    # four, and the bound is the lower-bound fall-back (no candidate of the chunk was left)
    def claim(t):
        for j in range(8):
            p = _panel(t, j)
            assert p["pick"] == "unit0" and p["gj"] == "kept" and p["chunks"] == 1 and p["units"][0]["stopped_early"] and p["per"] // 64 == 4
            assert p["new_first"] == 64 * j + 64 and p["route"] == "unit 0" and not p["wide"]
    C.append(_a("plain", 1, lambda sh, r: sh.plain(r, [7]), exact(unit0=8, gj_kept=8, chunks=8), claim))

    # gj_columns leaves 56 pivots: kept, and the second chunk's 8 rows go through the targeted path (8 columns missing).  The twin
    # leaves 55: redone row-wise, and 9 missing columns are one too many for the targeted path.  first_nonsrc is the first copy.
    def gj_twin(n):
        def write(sh, r):
            b = dense(r)
            sh.put(7, A_BASE, b[:n] + dense_copies(r, b[:n], 64 - n) + b[n:])

        def claim(t):
            p = _panel(t, 7)
            u0 = p["units"][0]
            assert p["pick"] == "unit0" and p["gj"] == ("kept" if n >= 56 else "redone") and p["chunks"] == 2
            assert u0["targeted"] == (1 if n >= 56 else 0) and p["new_first"] == A_BASE + n and p["p"] == 64
        return write, claim
    for n, kept in ((56, 1), (55, 0)):
        w, c = gj_twin(n)
        C.append(_a(f"gj_{n}_{'kept' if kept else 'redone'}", 2, w, exact(unit0=8, gj_kept=7 + kept, gj_redone=1 - kept, chunks=9), c))

    # the gate: 48 of the 64 words have more than 12 bits -> column-wise; 47 -> row-wise from the start.  The same 64 pivots
    def gate_twin(n):
        def write(sh, r):
            b = dense(r, n)
            sh.put(7, A_BASE, b + thin_independent(r, 64 - n, b))

        def claim(t):
            p = _panel(t, 7)
            assert p["pick"] == "unit0" and p["gj"] == ("kept" if n >= 48 else None) and p["chunks"] == 1 and p["p"] == 64
        return write, claim
    for n in (48, 47):
        w, c = gate_twin(n)
        C.append(_a(f"gate_{n}", 3, w, exact(unit0=8, gj_kept=7 + (n >= 48), chunks=8), c))

    # a candidate of the first chunk that is not taken: row 453 repeats row 451.  63 pivots from the first chunk, the 64th from the
    # second (targeted), and the bound is the copy's row
    def write(sh, r):
        b = dense(r)
        sh.put(7, A_BASE, b[:5] + [b[3]] + b[5:])

    def claim(t):
        p = _panel(t, 7)
        assert (p["pick"], p["gj"], p["chunks"], p["new_first"], p["route"]) == ("unit0", "kept", 2, A_BASE + 5, "unit 0")
        assert p["units"][0]["targeted"] == 1 and A_BASE + 5 not in p["srow"]
    C.append(_a("first_nonsrc_dup", 4, write, exact(unit0=8, gj_kept=8, chunks=9), claim))

    # unit 0 finds nothing, unit 3 is complete in its third chunk: adopted (pick = 3), and the bound advances from `first` -- where an
    # all-zero row stays alive
    def write(sh, r):
        sh.put(7, A_BASE + 3 * 256 + 128, dense(r))

    def claim(t):
        p = _panel(t, 7)
        assert (p["pick"], p["pick_at"], p["chunks"], p["gj"]) == ("unit", 3, 3, None) and p["units"][0]["cnt"] == 0
        assert p["route"] == "advance" and p["new_first"] == p["first"] == A_BASE and not p["hard"]
    C.append(_a("adopt_unit3", 5, write, exact(unit0=7, adopted=1, gj_kept=7, chunks=10), claim))

    # no unit is complete: lists of 40 + 40 + (empty) + 40.  The first 64 of the 120 rows have rank 40, the 16 rows that only the
    # carry keeps bring 16 more, the last list 8: rank 64 from 120 rows.  Rows 384 .. 423 are sources AND the rows at the old bound:
    # the new bound is 424, where panel 7 starts -- one chunk for it (row-wise: the panel is wide after a merge), two from 384
    def write(sh, r):
        a = stair(r, range(40), top=40)                         # unit 0: span V0, inside columns 0 .. 39
        sh.put(6, 384, a)
        new1, new3 = stair(r, range(40, 56)), stair(r, range(56, 64))
        sh.put(6, 640, [a[i] ^ a[i + 16] for i in range(24)] + new1)           # unit 1's list: 24 rows of V0 first, then 16 new ones
        sh.put(6, 1152, [a[i] ^ a[i + 8] for i in range(32)] + new3)           # unit 3's: 32 of V0, then the last 8
        sh.put(7, 424, dense(r))

    def claim(t):
        p, q = _panel(t, 6), _panel(t, 7)
        m = p["merge"]
        assert p["pick"] == "merge" and [u["cnt"] for u in p["units"]] == [40, 40, 0, 40, 0, 0, 0, 0]
        assert (m["sum"], m["carried"], m["cnt"], m["read"], m["empty"]) == (120, 16, 64, 8, 5) and p["hard"]
        assert p["first"] == 384 and p["new_first"] == 424 and p["route"] == "advance" and set(range(384, 424)) <= set(p["srow"])
        assert q["wide"] and q["pick"] == "unit0" and q["gj"] is None and q["chunks"] == 1
    C.append(_a("merge_carry_40_40_40", 6, write, exact(unit0=7, merged=1, wide=1, gj_kept=6, chunks=7), claim, special=6))

    # the merge is full after the first two lists (40 + 24 = one chunk exactly): the third, of 10 rows, is never read
    def write(sh, r):
        a = stair(r, range(40), top=40)
        sh.put(7, A_BASE, a)
        sh.put(7, A_BASE + 256, stair(r, range(40, 64)))
        sh.put(7, A_BASE + 768, [a[i] ^ a[i + 1] for i in range(10)])

    def claim(t):
        m = _panel(t, 7)["merge"]
        assert (m["read"], m["lists"], m["sum"], m["cnt"], m["carried"]) == (2, 8, 64, 64, 0) and _panel(t, 7)["units"][3]["cnt"] == 10
    C.append(_a("merge_full_early", 7, write, exact(unit0=7, merged=1, gj_kept=7, chunks=7), claim))

    # rank-deficient (20 + 20 rows, 10 of the second list inside the span of the first: p = 30), then a panel without a row (p = 0),
    # each merged and hard; panel 7 is wide after them
    def write(sh, r):
        a = stair(r, range(20), top=20)
        sh.put(5, 320, a)
        sh.put(5, 320 + 256, [a[i] ^ a[i + 10] for i in range(10)] + stair(r, range(30, 40)))
        sh.put(7, 340, dense(r))

    def claim(t):
        p5, p6, p7 = (_panel(t, j) for j in (5, 6, 7))
        assert (p5["pick"], p5["p"], p5["merge"]["sum"], p5["hard"]) == ("merge", 30, 40, True)
        assert (p6["pick"], p6["p"], p6["wide"], p6["hard"], p6["merge"]["empty"]) == ("merge", 0, True, True, 8)
        assert p5["new_first"] == p6["new_first"] == 340 and p7["wide"] and p7["pick"] == "unit0" and p7["gj"] is None
    C.append(_a("deficient_30_then_empty", 8, write, exact(unit0=6, merged=2, wide=2, gj_kept=5, chunks=6), claim, special=5))

    # 16 panels: the bound passes 512 after panel 7, so from panel 8 on the narrow workgroup of rows 256 .. 511 holds dead rows only
    # (dead_block) while workgroup 0, as dead, still stores the pivot rows; the first alive row is the one AT the bound
    rng = random.Random(9)
    sh = Sheet(2048, 1024)
    sh.plain(rng, range(16))

    def claim(t):
        assert [p["new_first"] for p in t["trace"]] == [64 * j + 64 for j in range(16)] and narrow_rpt(2048) == 1
    C.append(Case("dead_blocks_1024", 1024, sh.rows, exact(unit0=16, gj_kept=16, chunks=16), claim, seed=9))

    # `st->fast_off`, which a block's last general panel leaves for the dense block search of the NEXT block: 4 blocks, and the dense search
    # refuses block 0 in both twins (47 dense words in panel 2's chunk).  `cleared`: panel 3 is easy and full, fast_off = 0, and the dense
    # search takes blocks 1, 2, 3.  `stands`: panel 3 has 63 rows (merged, hard, p = 63), fast_off = 1, block 1 is not tried although
    # the dense search would take it (its rows follow at the bound, 255), its own last panel clears the flag, blocks 2 and 3 are taken
    def fast_off_twin(stands):
        rng = random.Random(16)
        sh = Sheet(2048, 1024)
        sh.plain(rng, [0, 1])
        b = dense(rng, 47)
        sh.put(2, 128, b + thin_independent(rng, 17, b))
        sh.put(3, 192, dense(rng)[:63 if stands else 64])
        sh.plain(rng, range(4, 16), at=255 if stands else 256)

        def claim(t):
            p3 = _panel(t, 3)
            assert (p3["pick"], p3["p"], p3["hard"], p3["fast_off"]) == (("merge", 63, True, 1) if stands else ("unit0", 64, False, 0))
            assert p3["new_first"] == (255 if stands else 256) and _panel(t, 7)["fast_off"] == 0
        e = exact(unit0=15, merged=1, wide=1, gj_kept=13, chunks=15) if stands else exact(unit0=16, gj_kept=15, chunks=16)
        return Case("fast_off_" + ("stands" if stands else "cleared"), 1024, sh.rows, e, claim, seed=16)
    C.append(fast_off_twin(False))
    C.append(fast_off_twin(True))

    # ---- more than 16 units ---------------------------------------------------------------------------------------------------------
    # 5000 rows, 20 units (groups of 16 and 4), 5 panels (a block of four and a block of one).  Panel 0: unit 0 is complete in its
    # ninth chunk -> hard.  Panel 1, two-level: unit 5 is complete, its group adopts it, the publisher adopts the group's record.
    # Panel 2: 20 rows, merged.  Panel 3, two-level: units 2 and 3 hold 32 rows each, their group's merge is complete and the
    # publisher adopts it -- a merged record is hard.  Panel 4, two-level: 40 rows in group 0, 24 in group 1, the publisher merges
    rng = random.Random(10)
    sh = Sheet(5000, 320)
    b = dense(rng)
    sh.put(0, 0, b[:63])
    sh.put(0, 517, b[63:])
    sh.put(1, 63 + 5 * 256, dense(rng))
    sh.put(2, 100, stair(rng, range(20)))
    s3 = stair(rng, range(64))
    sh.put(3, 600, s3[:32])
    sh.put(3, 850, s3[32:])
    s4 = stair(rng, range(64))
    sh.put(4, 330, s4[:40])
    sh.put(4, 4420, s4[40:])

    def claim(t):
        p = t["trace"]
        assert t["units"] == 20 and all(q["first"] == 63 for q in p[1:])
        assert (p[0]["pick"], p[0]["chunks"], p[0]["hard"], p[0]["gj"], p[0]["per"]) == ("unit0", 9, True, "kept", 640)
        assert p[1]["two_level"] and [g["how"] for g in p[1]["groups"]] == ["adopt", "merge"] and [g["size"] for g in p[1]["groups"]] == [16, 4]
        assert (p[1]["pick"], p[1]["pick_at"], p[1]["chunks"], p[1]["hard"], p[1]["per"]) == ("group", 0, 1, False, 256)
        assert (p[2]["pick"], p[2]["p"], p[2]["two_level"], p[2]["wide"]) == ("merge", 20, False, False)
        assert p[3]["two_level"] and p[3]["groups"][0]["how"] == "merge" and p[3]["groups"][0]["merge"]["sum"] == 64
        assert (p[3]["pick"], p[3]["pick_at"], p[3]["chunks"], p[3]["hard"]) == ("group", 0, MERGED_CHUNKS, True)
        assert p[4]["two_level"] and [g["cnt"] for g in p[4]["groups"]] == [40, 24] and (p[4]["pick"], p[4]["p"]) == ("merge", 64)
    C.append(Case("two_level_20_units", 320, sh.rows, exact(unit0=1, adopted=2, merged=2, wide=3, two_level=3, group_adopted=1, group_merged=5,
                                                             gj_kept=1, chunks=10), claim, seed=10))

    # 4352 rows, 17 units: the last group is unit 16 alone.  65 columns: panel 1 has ONE column (colmask = 1).  Panel 0 is hard (ninth
    # chunk); on panel 1 the only row with the bit lies in unit 16's slice: the group of one adopts its member, the publisher the group
    rng = random.Random(11)
    sh = Sheet(4352, 65)
    b = dense(rng)
    sh.put(0, 0, b[:63])
    sh.put(0, 520, b[63:])
    sh.put(1, 63 + 16 * 256 + 70, [1])

    def claim(t):
        p = t["trace"]
        assert t["units"] == 17 and p[0]["hard"] and p[0]["per"] == 576 and p[0]["chunks"] == 9
        assert p[1]["full"] == 1 and p[1]["two_level"] and [(g["how"], g["size"]) for g in p[1]["groups"]] == [("merge", 16), ("adopt", 1)]
        assert (p[1]["pick"], p[1]["pick_at"], p[1]["p"], p[1]["chunks"]) == ("group", 1, 1, 2)
    C.append(Case("group_of_one_65", 65, sh.rows, exact(unit0=1, adopted=1, wide=1, two_level=1, group_adopted=1, group_merged=1, gj_kept=1,
                                                         chunks=11), claim, seed=11))

    # 129 columns: panel 2 has one column.  Panel 1 is rank-deficient (hard); on panel 2, two-level, UNIT 0 is complete: the publisher
    # takes unit 0's own record past the groups (and its bound).  A unit of a wide panel never runs gj_columns, so it never has the
    # column slots that self-publication wants: `!(wide && units > GF2_GROUP)` in `self` refuses nothing that `S.colslots` has not
    rng = random.Random(12)
    sh = Sheet(4352, 129)
    sh.plain(rng, [0])
    sh.put(1, 64, stair(rng, range(50)))
    sh.put(2, 130, [1, 1])

    def claim(t):
        p = t["trace"]
        assert (p[1]["pick"], p[1]["p"], p[1]["hard"]) == ("merge", 50, True)
        assert p[2]["two_level"] and (p[2]["pick"], p[2]["full"], p[2]["p"], p[2]["route"], p[2]["gj"]) == ("unit0", 1, 1, "unit 0", None)
        assert [g["how"] for g in p[2]["groups"]] == ["adopt", "merge"] and p[2]["new_first"] == 114
    C.append(Case("unit0_two_level_129", 129, sh.rows, exact(unit0=2, merged=1, wide=1, two_level=1, group_adopted=1, group_merged=1, gj_kept=1,
                                                              chunks=1 + 1), claim, seed=12))

    # 100 columns: panel 1 has 36 (colmask = 2^36 - 1): never column-wise, complete at 36 pivots
    rng = random.Random(13)
    sh = Sheet(4352, 100)
    sh.plain(rng, [0])
    w36 = []
    while len(w36) < 36:
        w = rng.getrandbits(36)
        if rank_of(w36 + [w]) == len(w36) + 1:
            w36.append(w)
    sh.put(1, 64, w36 + copies(rng, w36, 20))

    def claim(t):
        p = t["trace"][1]
        assert (p["full"], p["pick"], p["p"], p["gj"], p["chunks"], p["new_first"]) == (36, "unit0", 36, None, 1, 100)
    C.append(Case("colmask_36_of_100", 100, sh.rows, exact(unit0=2, gj_kept=1, chunks=2), claim, seed=13))

    # ---- tall: 131328 rows = 256 units, 16 groups of 16, two row blocks per narrow workgroup ----------------------------------------
    # panel 0 hard (tenth chunk of unit 0's 257); panel 1: unit 100 complete, group 6 adopts, the other 15 merge nothing; panel 2 has
    # no row (hard); panel 3: four rows in unit 16 g + 1 of groups 0 .. 13, eight in group 14, 16 group merges and the publisher's merge of their lists;
    # panel 4: unit 0 complete under the two-level arrival (its group adopts it, the publisher takes unit 0's own record); panels 5 .. 7 by unit 0 again, narrow
    rng = random.Random(14)
    sh = Sheet(131328, 512)
    b = dense(rng)
    sh.put(0, 0, b[:63])
    sh.put(0, 600, b[63:])
    sh.put(1, 63 + 576 * 100, dense(rng))
    s3 = stair(rng, range(64))
    for g in range(15):                     # (per = 576 rows: the slices of units 228 .. 255, group 15 among them, are empty)
        sh.put(3, 63 + 576 * (16 * g + 1) + 8, s3[4 * g:4 * g + 4] if g < 14 else s3[56:])
    sh.plain(rng, [4, 5, 6, 7], at=64)

    def claim(t):
        p = t["trace"]
        assert t["units"] == 256 and narrow_rpt(131328) == 2 and all(q["first"] == 63 for q in p[1:])
        assert (p[0]["pick"], p[0]["chunks"], p[0]["hard"], p[0]["active"]) == ("unit0", 10, True, 8)
        assert p[1]["active"] == 256 and p[1]["per"] == 576 and [g["how"] for g in p[1]["groups"]] == ["merge"] * 6 + ["adopt"] + ["merge"] * 9
        assert (p[1]["pick"], p[1]["pick_at"], p[1]["hard"]) == ("group", 6, False)
        assert (p[2]["pick"], p[2]["p"], p[2]["two_level"]) == ("merge", 0, False)
        assert p[3]["two_level"] and [g["cnt"] for g in p[3]["groups"]] == [4] * 14 + [8, 0] and (p[3]["pick"], p[3]["p"]) == ("merge", 64)
        assert p[4]["two_level"] and (p[4]["pick"], p[4]["chunks"], p[4]["hard"]) == ("unit0", 2, False)
        assert [q["wide"] for q in p[5:]] == [False] * 3 and all(q["pick"] == "unit0" for q in p[5:])
    C.append(Case("tall_256_units", 512, sh.rows, exact(unit0=5, adopted=1, merged=2, wide=3, two_level=3, group_adopted=1 + 1, group_merged=15 + 16 + 15,
                                                         gj_kept=1, chunks=10 + 1 + 2 + 3 + 4 + 5), claim, seed=14, tall=True))

    # tall and plain: all 512 sources are rows 0 .. 511, so the last narrow step meets a bound of 512 and a narrow workgroup's SECOND
    # row block (rows 256 .. 511 of workgroup 0) holds dead rows only (dead_rows), its first the sources' block that is kept
    rng = random.Random(15)
    sh = Sheet(131328, 512)
    sh.plain(rng, range(8))

    def claim(t):
        assert [q["new_first"] for q in t["trace"]] == [64 * j + 64 for j in range(8)] and narrow_rpt(131328) == 2
    C.append(Case("tall_plain", 512, sh.rows, exact(unit0=8, gj_kept=8, chunks=8), claim, seed=15, tall=True))
    return C


_CASES = None


def cases() -> dict:
    """name -> Case, built once"""
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in all_cases()}
    return _CASES


NAMES = ["plain", "gj_56_kept", "gj_55_redone", "gate_48", "gate_47", "first_nonsrc_dup", "adopt_unit3", "merge_carry_40_40_40",
         "merge_full_early", "deficient_30_then_empty", "dead_blocks_1024", "fast_off_cleared", "fast_off_stands", "two_level_20_units", "group_of_one_65", "unit0_two_level_129",
         "colmask_36_of_100", "tall_256_units", "tall_plain"]

# the twins: (one, the other, the counters in which -- and only in which -- their predictions differ)
TWINS = [("gj_56_kept", "gj_55_redone", {"general_gj_kept", "general_gj_redone"}), ("gate_48", "gate_47", {"general_gj_kept"})]

# the four mutants of profiles/general_search_mutants.txt as switches of `simulate`, and a case each must move
MUTANTS = {"no carry": ({"carry": False}, "merge_carry_40_40_40"), "GF2_GROUP 8": ({"group": 8}, "two_level_20_units"),
           "GF2_FEW_UNITS 4": ({"few_units": 4}, "adopt_unit3"), "bound keeps own sources": ({"exclude_sources": False}, "merge_carry_40_40_40")}
