"""Built systems for the one-launch small solve (k_small_solve) and what each must trigger, with a plain-integer model of the
kernel's passes (inputs and the model only -- no solver here).

The kernel works panel by panel (64 columns = one word).  A PASS gathers up to 64 candidate rows -- rows that are no pivots and have
a bit in a pivot-less column of the panel -- reduces their words of the panel against each other column by column (ascending; the first
unused candidate that has the bit becomes the column's pivot), and every other row then takes the new pivot rows its bits select.  A pass
that found at most 4 pivots runs bit loops on the rows themselves, one that found more builds nibble tables.  Passes repeat until a pass
finds no candidate.  gf2bv_stats::small_passes counts the passes, small_pass_kinds says which kinds ran (KIND_* below).

Which 64 candidates a pass takes is a race.  Wavefront wv looks at the STRIPE rows 64 wv + 1024 i .. + 63 in its iteration i, adds the
number of its candidates to one counter (atomicAdd: the old value is its first slot, candidates enter in lane order while slots are
left) and goes on to iteration i + 1 only if the counter is below 64 when it looks.  The answers are the RREF's whatever was taken; the
two counters are not.  The cases here are built so that every arrival order gives the same passes and kinds:

  (F) FULL stripes: every stripe among rows 0..1023 holds 64 candidates.  A pass then takes exactly ONE whole stripe, whichever wins
      (the first add takes the counter to 64), and rows >= 1024 are not looked at in that pass: a wavefront's own add of 64 precedes
      its second look.  Every stripe must lead to the same (pivots found, candidates left for the next pass).
  (A) ALL in: a pass whose candidates number at most 64 takes every one of them, whatever the order and wherever they are (only
      their slots differ) -- rows >= 1024 included.
  (S) identical stripes (slots_40): the winner's 40 candidates and the next wavefront's first 24 are the same vectors whoever they are.
  A case whose stripes are only PARTLY filled with candidates and hold more than 64 in all puts no candidate at rows >= 1024: a fast
  wavefront's second iteration could overtake a slow one's first, and the arrival orders modelled here would not cover it
  (`check_construction`).

Rows whose coefficient support lies inside one panel are never changed by another panel's elimination, so the panels of such a system
are independent of each other and each meets exactly what was written here ("confined" cases: counters EXACT).  The "mixed" cases put
the designed panel FIRST and give every row random bits in all later words, so the candidates' other words follow the combinations
and the all-rows step carries real data; their later panels are ordinary, so the counters only CONTAIN the designed ones
(passes >=, kinds a superset).

Bit 4 (a pass left candidates out) in the (F) cases rests on one more premise than the arrival order: at least two wavefronts make their
first look before the first add lands.  They leave the same barrier, and an add follows its look by an LDS round trip, a ballot and the
atomic itself, so the model's default (`serial=False`: every wavefront's first look precedes every add) is what the hardware does; the
CPU file also runs every case with `serial=True` (each wavefront finishes before the next looks) and requires passes, rank and every
other kind bit to be the same.

Shapes: the single-system entries refuse rows < cols (check_shape, as the reference), so an eligible system -- (rows + 512) x (wt | 1)
<= 18432 words, cols <= 1023, rows <= 4096 -- has at most 13 words per row: 14 words (cols >= 832) would need rows <= 716.  The
kernel's room for 14-16 words (SmallLds::have[16], MAXI) is not reachable through the entries; tests/test_small_cases_cpu.py states
that and `wide13` is the widest case.

tests/test_small_cases_cpu.py checks the premises per case; tests/test_gpu_small_cases.py runs the cases."""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np

NT = 1024                        # threads of k_small_solve as small_solve launches it
NW = NT // 64                    # wavefronts: a stripe each per iteration
LDS_WORDS, MAXROWS, MAXCOLS = 18432, 4096, 1023      # small_eligible

KIND_FIRST_FEW, KIND_FIRST_TABLES, KIND_LATER_FEW, KIND_LATER_TABLES, KIND_LEFT_OUT, KIND_UNDER_64 = 1, 2, 4, 8, 16, 32

M64 = (1 << 64) - 1


def words_of(cols: int) -> int:
    return (cols + 1 + 63) // 64


def eligible(rows: int, cols: int) -> bool:
    """small_eligible: matrix + 2 x 256 table entries at an odd row pitch in 18432 words of LDS"""
    return cols <= MAXCOLS and rows <= MAXROWS and (rows + 512) * (words_of(cols) | 1) <= LDS_WORDS


def largest_rows(wt: int) -> int:
    """the most rows a system of wt words per row may have and be eligible"""
    return min(MAXROWS, LDS_WORDS // (wt | 1) - 512)


def e(i: int) -> int:
    return 1 << i


def digits(eqs, bpd: int):
    """CPython's digits of non-negative equation integers at bpd bits per digit, as gf2bv_solve_digits takes them: (uint32 digits, int64
    offsets); 0 has NO digits (off[r + 1] == off[r], as CPython's 0)"""
    nd = [(v.bit_length() + bpd - 1) // bpd for v in eqs]
    off = np.zeros(len(eqs) + 1, dtype=np.int64)
    np.cumsum(nd, out=off[1:])
    dig = np.zeros(int(off[-1]), dtype=np.uint32)
    for i, v in enumerate(eqs):
        k = int(off[i])
        while v:
            dig[k] = v & ((1 << bpd) - 1)
            v >>= bpd
            k += 1
    return dig, off


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def gather(cand_of_stripe, rows: int, order, serial: bool):
    """The slot race of one pass.  cand_of_stripe(r0) = the candidate rows among r0 .. r0 + 63 in lane order.  `order`: the wavefronts
    in arrival order.  serial False: iteration 0 of every wavefront (all looked before any add), then iteration 1 in the same order, each
    looking (counter < 64?) right before its add, and so on.  serial True: each wavefront runs all its iterations before the next looks
    for the first time.  Returns (list of at most 64 rows in slot order, ncand)."""
    lst, ncand = [], 0

    def add(wv, it):
        nonlocal ncand
        c = cand_of_stripe(64 * wv + NT * it)
        lst.extend(c[:max(0, 64 - ncand)])
        ncand += len(c)

    if serial:
        for wv in order:
            it = 0
            while 64 * wv + NT * it < rows and ncand < 64:
                add(wv, it)
                it += 1
    else:
        it = 0
        while any(64 * wv + NT * it < rows for wv in order):
            for wv in order:
                if 64 * wv + NT * it < rows and (it == 0 or ncand < 64):
                    add(wv, it)
            it += 1
            if ncand >= 64:
                break
    return lst, ncand


def model(coef_rows, cols: int, order=None, serial: bool = False, panels: int | None = None) -> dict:
    """One solve as k_small_solve is written, on whole rows as integers (bit c = column c; the constant plays no part in the passes).
    `panels`: stop after that many panels.  Returns passes, kinds, rank, pivrow (column -> its pivot row), per_panel (the passes of each panel)."""
    order = list(range(NW)) if order is None else list(order)
    assert sorted(order) == list(range(NW))
    A = list(coef_rows)
    rows = len(A)
    rowpiv = [-1] * rows
    pivrow = {}
    passes = kinds = 0
    per_panel = []
    npan = (cols + 63) // 64
    for q in range(npan if panels is None else min(panels, npan)):
        colmask = M64 if cols - 64 * q >= 64 else e(cols - 64 * q) - 1
        have, first, p0 = 0, True, passes
        while True:
            opn = colmask & ~have
            if not opn:
                break

            def cand_of_stripe(r0):
                return [r for r in range(r0, min(r0 + 64, rows)) if rowpiv[r] < 0 and (A[r] >> (64 * q)) & opn]

            lst, ncand = gather(cand_of_stripe, rows, order, serial)
            n = min(ncand, 64)
            if n == 0:
                break
            passes += 1
            # column by column, ascending: the first unused candidate with the bit is the pivot, every other candidate with it takes it
            used, newrow = set(), {}
            for b in range(64):
                if not (colmask >> b) & 1:
                    continue
                L = next((i for i in range(n) if i not in used and (A[lst[i]] >> (64 * q + b)) & 1), None)
                if L is None:
                    continue
                used.add(L)
                newrow[b] = lst[L]
                for i in range(n):
                    if i != L and (A[lst[i]] >> (64 * q + b)) & 1:
                        A[lst[i]] ^= A[lst[L]]
            nm = sum(e(b) for b in newrow)
            assert nm and not nm & ~opn
            kinds |= (KIND_FIRST_FEW if len(newrow) <= 4 else KIND_FIRST_TABLES) << (0 if first else 2)
            if ncand > 64:
                kinds |= KIND_LEFT_OUT
            if n < 64:
                kinds |= KIND_UNDER_64
            for b, r in newrow.items():
                rowpiv[r] = 64 * q + b
                pivrow[64 * q + b] = r
            # every other row takes the new pivot rows its bits select
            pr = set(newrow.values())
            for r in range(rows):
                if r in pr:
                    continue
                m = (A[r] >> (64 * q)) & nm
                while m:
                    b = (m & -m).bit_length() - 1
                    m &= m - 1
                    A[r] ^= A[newrow[b]]
            have |= nm
            first = False
        per_panel.append(passes - p0)
    return {"passes": passes, "kinds": kinds, "rank": len(pivrow), "pivrow": pivrow, "per_panel": per_panel}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    cols: int
    coef: list                   # row -> coefficient integer (bit c = column c)
    passes: int                  # the designed passes ...
    kinds: int                   # ... and kinds: of the whole solve (exact) or of the designed panel (mixed: contained)
    exact: bool                  # True: small_passes == passes and small_pass_kinds == kinds; False: >= and superset
    rule: str                    # "F" full stripes (one winner per pass), "A" all in / "S" identical stripes
    panel: int = 0               # the designed panel
    plant: int = 0               # the planted solution the constants follow

    @property
    def rows(self) -> int:
        return len(self.coef)

    @property
    def mixed(self) -> bool:
        return not self.exact

    def eqs(self) -> list:
        """equation integers: bit 0 = constant, bit k = coefficient of variable k - 1"""
        return [(a << 1) | (bin(a & self.plant).count("1") & 1) for a in self.coef]

    def aug(self) -> np.ndarray:
        wt = words_of(self.cols)
        out = np.zeros((self.rows, wt), dtype=np.uint64)
        for r, a in enumerate(self.coef):
            v = a | ((bin(a & self.plant).count("1") & 1) << self.cols)
            out[r] = np.frombuffer(v.to_bytes(8 * wt, "little"), dtype=np.uint64)
        return out

    def orders(self, shuffles: int = 200) -> list:
        """the arrival orders to enumerate: each stripe of rows 0..1023 as the winner for the full-stripe cases (what follows the winner
        adds nothing), identity, reverse and seeded shuffles for the others"""
        ident = list(range(NW))
        if self.rule == "F":
            nst = min(NW, (self.rows + 63) // 64)
            out = [[s] + [w for w in ident if w != s] for s in range(nst)] + [ident[::-1]]
            if self.rows < 1024 and self.rows % 64:      # a shorter last stripe does not fill the slots: every second arrival behind it
                out += [[nst - 1, t] + [w for w in ident if w not in (nst - 1, t)] for t in range(nst - 1)]
            return out
        rng = random.Random(sum(map(ord, self.name)))
        out = [ident, ident[::-1]]
        for _ in range(shuffles):
            o = ident[:]
            rng.shuffle(o)
            out.append(o)
        return out

    def holds(self, passes: int, kinds: int) -> bool:
        if self.exact:
            return passes == self.passes and kinds == self.kinds
        return passes >= self.passes and kinds & self.kinds == self.kinds


def span_rows(rng: random.Random, cols_of_span: list, n: int, units_at: int) -> list:
    """n non-zero rows from the span of the unit vectors of `cols_of_span`: the sum of all of them first, random combinations, and the
    unit vectors themselves from lane `units_at` on (so pivots are formed from combinations, not found ready-made)"""
    k = len(cols_of_span)
    full = sum(e(c) for c in cols_of_span)
    out = [full]
    while len(out) < n:
        x = rng.randrange(1, 1 << k)
        out.append(sum(e(c) for i, c in enumerate(cols_of_span) if (x >> i) & 1))
    for i, c in enumerate(cols_of_span):
        out[units_at + i] = e(c)
    return out


def independent_rows(rng: random.Random, lo: int, n: int, width: int | None = None) -> list:
    """n independent rows with support in columns lo .. lo + width - 1 (width defaults to n): a random invertible mix, so the rows
    carry real combinations"""
    width = n if width is None else width
    rowsv, basis = [], {}
    while len(rowsv) < n:
        w = v = rng.getrandbits(width)
        while v:
            h = v.bit_length() - 1
            if h not in basis:
                basis[h] = v
                rowsv.append(w << lo)
                break
            v ^= basis[h]
    return rowsv


def randomise_later_words(rng: random.Random, coef: list, cols: int, first_word: int = 1) -> list:
    """the mixed cases: every row gets random bits in all words from `first_word` on"""
    out = []
    for a in coef:
        hi = rng.getrandbits(cols - 64 * first_word) << (64 * first_word)
        out.append((a & (e(64 * first_word) - 1)) | hi)
    return out


def _first_k(rng, k, rows, units_at=20):
    """every stripe full of candidates from a k-dimensional span of panel 0's columns; each stripe holds the unit rows"""
    span = [3 + 7 * i for i in range(k)]
    coef = []
    for r0 in range(0, rows, 64):
        coef += span_rows(rng, span, 64, units_at)
    return coef[:rows], span


def _later_own_columns(rng, rows, own):
    """Full stripes for a second pass below 1024 rows: every stripe spans columns 0..31 (e0..e31 and 28 combinations), and stripe s < own
    also carries its OWN column 32 + s in two rows (the unit and a sum).  Pass 1 takes one stripe: 32 or 33 pivots through the tables.
    Pass 2 finds the other stripes' own rows -- at most 2 x own candidates, all in -- and `own` or `own - 1` pivots."""
    coef = []
    base = list(range(32))
    for s, r0 in enumerate(range(0, rows, 64)):
        st = span_rows(rng, base, 64, 12)
        if s < own:
            st[50] = e(32 + s)
            st[51] = e(32 + s) ^ e(3) ^ e(17)
        coef += st
    return coef[:rows]


def cases() -> dict:
    """name -> Case, in the order of NAMES"""
    out = {}
    PLANT_LOW = M64      # the planted solution is 1 in every column of panel 0: a row left with a stray bit there shows in its constant

    def add(name, cols, coef, passes, kinds, exact, rule, panel=0, plant=None):
        rng = random.Random(1000 + len(out))
        out[name] = Case(name, cols, coef, passes, kinds, exact, rule, panel, rng.getrandbits(cols) | PLANT_LOW if plant is None else plant)

    # one_pass_64: 64 independent rows per panel, every 17th row (many stripes, both iterations), everything else zero
    rng = random.Random(11)
    coef = [0] * 1088
    for q, shift in ((0, 0), (1, 5)):
        for i, w in enumerate(independent_rows(rng, 64 * q, 64)):
            coef[17 * i + shift] = w
    add("one_pass_64", 128, coef, 2, KIND_FIRST_TABLES, True, "A")

    # first_3 / first_4 / first_5: the 4 / 5 edge of the bit loops against the tables
    for k in (3, 4, 5):
        coef, _ = _first_k(random.Random(20 + k), k, 640)
        add(f"first_{k}", 100, coef, 1, (KIND_FIRST_FEW if k <= 4 else KIND_FIRST_TABLES) | KIND_LEFT_OUT, True, "F")

    # later_tables: stripes 0-15 are e0..e31 twice, rows 1024-1087 e32..e63 twice: two passes of 32 pivots, the second from a second stripe
    rng = random.Random(31)
    coef = []
    for s in range(17):
        st = [e(i + (32 if s == 16 else 0)) for i in range(32)] * 2
        rng.shuffle(st)
        coef += st
    add("later_tables", 64, coef, 2, KIND_FIRST_TABLES | KIND_LATER_TABLES | KIND_LEFT_OUT, True, "F")

    # later_few: every stripe below 1024 spans columns 0-61 with two sums among its rows; rows >= 1024 carry columns 62 and 63
    rng = random.Random(32)
    coef = []
    for s in range(16):
        st = [e(i) for i in range(62)] + [e(0) ^ e(5), e(7) ^ e(61) ^ e(30)]
        rng.shuffle(st)
        coef += st
    coef += [e(62), e(63) ^ e(62), e(62)]
    add("later_few", 64, coef, 2, KIND_FIRST_TABLES | KIND_LATER_FEW | KIND_LEFT_OUT | KIND_UNDER_64, True, "F")

    # slots_40: every stripe holds the same 40 independent vectors in lanes 0-39 and zero rows behind them
    rng = random.Random(33)
    v = independent_rows(rng, 0, 40, 64)
    add("slots_40", 70, (v + [0] * 24) * 8, 1, KIND_FIRST_TABLES | KIND_LEFT_OUT, True, "S")

    # second_stripe_first_pass: 20 candidates below row 1024, 40 at rows >= 1024 in two wavefronts' second stripes: 60 in all, all in
    rng = random.Random(34)
    v = independent_rows(rng, 0, 60, 64)
    coef = [0] * 1160
    for i in range(20):
        coef[53 * i + 7] = v[i]
    for i in range(40):
        coef[1030 + 3 * i] = v[20 + i]
    add("second_stripe_first_pass", 64, coef, 1, KIND_FIRST_TABLES | KIND_UNDER_64, True, "A")

    # last_stripe_4096: the only candidates are in rows 4032-4095, wavefront 15's fourth iteration
    rng = random.Random(35)
    coef = [0] * 4032 + independent_rows(rng, 0, 40, 64) + independent_rows(rng, 64, 24, 36)
    add("last_stripe_4096", 100, coef, 2, KIND_FIRST_TABLES | KIND_UNDER_64, True, "A")

    # deficient_then_empty: a panel of rank 30 (50 rows, all in), a panel with no bit at all (no pass), a full one
    rng = random.Random(36)
    b30 = independent_rows(rng, 2, 30, 60)
    coef = [0] * 300
    for i in range(50):
        coef[6 * i + 1] = b30[i] if i < 30 else b30[rng.randrange(30)] ^ b30[rng.randrange(30)] ^ b30[0]
    for i, w in enumerate(independent_rows(rng, 128, 64)):
        coef[4 * i + 2] = w
    add("deficient_then_empty", 192, coef, 2, KIND_FIRST_TABLES | KIND_UNDER_64, True, "A")

    # partial_last_panel: cols % 64 = 1 and 63 with the designed panel last -- colmask and the constant in the same word (63: at bit 63)
    rng = random.Random(37)
    coef = [0] * 140
    for i, w in enumerate(independent_rows(rng, 0, 64)):
        coef[2 * i] = w
    for i in range(10):
        coef[14 * i + 1] = e(64)
    add("partial_last_1", 65, coef, 2, KIND_FIRST_TABLES | KIND_FIRST_FEW | KIND_UNDER_64, True, "A", panel=1)
    coef = [0] * 140
    for i, w in enumerate(independent_rows(rng, 0, 64)):
        coef[2 * i] = w
    for i, w in enumerate(independent_rows(rng, 64, 63)):
        coef[2 * i + 1] = w
    add("partial_last_63", 127, coef, 2, KIND_FIRST_TABLES | KIND_UNDER_64, True, "A", panel=1)

    # mixed: the designed panel first, random bits in every later word; the widest eligible shape (13 words: 905 x 831)
    rows13, cols13 = largest_rows(13), 64 * 13 - 1
    rng = random.Random(41)
    coef, _ = _first_k(rng, 3, rows13)
    add("wide13_first_3", cols13, randomise_later_words(rng, coef, cols13), 1, KIND_FIRST_FEW | KIND_LEFT_OUT, False, "F")
    rng = random.Random(42)
    coef, _ = _first_k(rng, 5, rows13)
    add("wide13_first_5", cols13, randomise_later_words(rng, coef, cols13), 1, KIND_FIRST_TABLES | KIND_LEFT_OUT, False, "F")
    rng = random.Random(43)
    add("wide13_later_tables", cols13, randomise_later_words(rng, _later_own_columns(rng, rows13, 9), cols13), 2,
        KIND_FIRST_TABLES | KIND_LATER_TABLES | KIND_LEFT_OUT | KIND_UNDER_64, False, "F")
    rng = random.Random(44)
    add("wide13_later_few", cols13, randomise_later_words(rng, _later_own_columns(rng, rows13, 4), cols13), 2,
        KIND_FIRST_TABLES | KIND_LATER_FEW | KIND_LEFT_OUT | KIND_UNDER_64, False, "F")
    # ... and 12 words at its largest row count (the row pitch is 13 words for both: 12 | 1)
    rows12, cols12 = largest_rows(12), 64 * 12 - 1
    rng = random.Random(45)
    coef, _ = _first_k(rng, 4, rows12)
    add("wide12_first_4", cols12, randomise_later_words(rng, coef, cols12), 1, KIND_FIRST_FEW | KIND_LEFT_OUT, False, "F")
    return out


NAMES = ["one_pass_64", "first_3", "first_4", "first_5", "later_tables", "later_few", "slots_40", "second_stripe_first_pass",
         "last_stripe_4096", "deficient_then_empty", "partial_last_1", "partial_last_63",
         "wide13_first_3", "wide13_first_5", "wide13_later_tables", "wide13_later_few", "wide12_first_4"]


def check_construction(case: Case):
    """The construction rule, on the panel words as written (pass 1 of each panel of a confined case, the designed panel of a mixed one):
    a panel whose stripes are only partly filled with candidates and hold more than 64 in all has no candidate at rows >= 1024; a
    full-stripe panel has 64 candidates in EVERY stripe below row 1024 (the last, shorter stripe of the matrix excepted)."""
    npan = (case.cols + 63) // 64
    for q in ([case.panel] if case.mixed else range(npan)):
        per = {}
        for r, a in enumerate(case.coef):
            if (a >> (64 * q)) & M64:
                per[r // 64] = per.get(r // 64, 0) + 1
        if not per:
            continue
        total, low = sum(per.values()), [per.get(s, 0) for s in range(min(NW, (case.rows + 63) // 64))]
        whole = low[:-1] if case.rows < 1024 and case.rows % 64 else low
        if all(c == 64 for c in whole) and whole:
            continue                                   # (F)
        if total <= 64:
            continue                                   # (A)
        assert not any(s >= NW for s in per), (case.name, q, "partly filled stripes, more than 64 candidates, and some at rows >= 1024")
