"""The job tables of tests/test_gpu_threads.py and tests/threads_child.py: one builder per entry group, each returning jobs
(name, callable, want) for tests/threads.run_concurrently.

Building a job touches no device: the inputs come from the generators of the single-thread tests at their smallest shapes, and every
`want` from a reference outside the library -- the CPU oracle for the solves, the set-of-monomials helpers for the expansions, the
zero sets known by construction for the searches.  (The plan jobs are the exception: their reference is the library's host twin,
as in the single-thread tests.)  A callable makes ONE library call -- two for the device-resident pair -- and returns its result as a
plain comparable value."""
from __future__ import annotations

import itertools
import random
import threading

import numpy as np

from gf2bv_amd import QuadraticSystem, hip
from gf2bv_amd.linsys import xl3_cols, xl4_cols
from oracle import gf2_oracle as O
from tests import cubic_forms as CF
from tests import quad_forms as QF
from tests import quartic_forms as Q4F
from tests import threads as T
from tests import xl4_terms as X4
from tests import xl_guess_terms as G
from tests import xl_terms as X
from tests.quad_terms import expand_ints, random_terms, to_aug
from tests.systems import random_system

SENTINEL = 0x5A5A5A5A5A5A5A5A


# -- helpers that tests/test_gpu_rhs.py and tests/test_gpu_quad_forms.py also have (kept here so that the child imports no test module)
def rhs_words(bits: np.ndarray) -> np.ndarray:
    """nrhs x rows 0/1 -> nrhs x ceil(rows/64) uint64, bit r of row j = bits[j, r]"""
    nrhs, rows = bits.shape
    rw = (rows + 63) // 64
    padded = np.zeros((nrhs, rw * 64), dtype=np.uint8)
    padded[:, :rows] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(nrhs, rw)


def coefficient_bits(aug: np.ndarray, rows: int, cols: int) -> np.ndarray:
    cw = (cols + 63) // 64
    by = np.ascontiguousarray(aug[:rows, :cw]).view(np.uint8).reshape(rows, cw * 8)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :cols]


def make_rhs(rng: random.Random, aug: np.ndarray, rows: int, cols: int, nrhs: int) -> np.ndarray:
    """nrhs x rows 0/1: the even ones planted (b = A x, consistent), the odd ones random"""
    A = coefficient_bits(aug, rows, cols).astype(np.int64)
    out = np.zeros((nrhs, rows), dtype=np.uint8)
    for j in range(nrhs):
        if j % 2 == 0:
            x = np.array([rng.getrandbits(1) for _ in range(cols)], dtype=np.int64)
            out[j] = (A @ x) & 1
        else:
            out[j] = [rng.getrandbits(1) for _ in range(rows)]
    return out


def with_rhs(aug: np.ndarray, cols: int, b: np.ndarray) -> np.ndarray:
    a = aug.copy()
    w, bit = cols // 64, np.uint64(cols % 64)
    a[:, w] = (a[:, w] & ~(np.uint64(1) << bit)) | (b.astype(np.uint64) << bit)
    return a


def oracle_rhs(aug, rows: int, cols: int, bits: np.ndarray, mode: int) -> tuple:
    """the CPU oracle's answer for every right-hand side of `bits`, as the keys solve_many returns"""
    return tuple(T.oracle_key(O.solve_words(with_rhs(aug, cols, b), rows, cols, mode), mode) for b in bits)


def solve_many(sols, mode: int) -> tuple:
    return tuple(T.solution_key(s, mode) for s in sols)


def pad_to(rng, forms, m: int) -> list:
    """the forms and XORs of two of them, m in all (the common zeros stay what they are)"""
    forms = list(forms)
    while len(forms) < m:
        if (m - len(forms)) % 2:
            a, b = rng.sample(range(min(8, len(forms))), 2)
            forms.insert(max(a, b) + 1, forms[a] ^ forms[b])
        else:
            a, b = rng.sample(range(len(forms)), 2)
            forms.append(forms[a] ^ forms[b])
    return forms


# -- the single-system, many-RHS and batch solves against the CPU oracle ---------------------------------------------------------------
def solve_jobs(seeds, rows: int, cols: int, cap, mode: int = 1) -> list:
    """hip.solve_words: 66 x 65 takes the one-launch path, 2600 x 2500 (rank cap 2300) the blocked path over several blocks"""
    jobs = []
    for s in seeds:
        rng = random.Random(1000 * rows + s)
        aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, cap if s % 2 == 0 or cap is not None else cols - 5, s % 4 != 3, 0), cols)
        want = T.oracle_key(O.solve_words(aug, rows, cols, mode), mode)
        jobs.append((f"solve_words {rows}x{cols} #{s}", lambda aug=aug: T.solution_key(hip.solve_words(aug, rows, cols, mode), mode), want))
    return jobs


def rhs_jobs(seeds, rows: int = 300, cols: int = 200, cap: int = 40, nrhs: int = 65, mode: int = 1) -> list:
    """hip.solve_rhs_words: 65 right-hand sides are two passes of 64 slots"""
    jobs = []
    for s in seeds:
        rng = random.Random(2000 + s)
        aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, cap, True, 0), cols)
        bits = make_rhs(rng, aug, rows, cols, nrhs)
        rhs = rhs_words(bits)
        jobs.append((f"solve_rhs_words {rows}x{cols} n{nrhs} #{s}",
                     lambda aug=aug, rhs=rhs: solve_many(hip.solve_rhs_words(aug, rows, cols, rhs, mode), mode),
                     oracle_rhs(aug, rows, cols, bits, mode)))
    return jobs


def batch_jobs(seeds, rows: int = 400, cols: int = 321, mode: int = 1) -> list:
    """hip.solve_batch_words: a gang of 3 (the shapes of test_batch_words_host_entry)"""
    jobs = []
    for s in seeds:
        rng = random.Random(3000 + s)
        systems = [random_system(rng, rows, cols, .5, cap) for cap in (None, 200, 1)]
        augs = np.stack([O.eqs_to_aug(e, cols) for e in systems])
        want = tuple(T.oracle_key(O.solve_words(a, rows, cols, mode), mode) for a in augs)
        jobs.append((f"solve_batch_words 3 x {rows}x{cols} #{s}", lambda augs=augs: solve_many(hip.solve_batch_words(augs, rows, cols, mode), mode), want))
    return jobs


def space_jobs(seeds, dim: int = 12, words: int = 17, count: int = 1024) -> list:
    """hip.space_enumerate in Gray order against the oracle's iteration order"""
    jobs = []
    for s in seeds:
        rng = random.Random(4000 + s)
        origin = np.array([rng.getrandbits(64) for _ in range(words)], dtype=np.uint64)
        basis = np.array([[rng.getrandbits(64) for _ in range(words)] for _ in range(dim)], dtype=np.uint64).reshape(dim, words)
        sp = O.OracleSpace(O.words_to_int(origin), tuple(O.words_to_int(b) for b in basis))
        want = np.stack([O.int_to_words(v, words) for v in itertools.islice(iter(sp), count)])
        jobs.append((f"space_enumerate dim {dim} #{s}", lambda origin=origin, basis=basis: hip.space_enumerate(origin, basis, 0, count, gray=True), want))
    return jobs


# -- the expansions against the set-of-monomials helpers ------------------------------------------------------------------------------------
def quad_expand_jobs(seeds, n: int = 65, rows: int = 13) -> list:
    q = QuadraticSystem([n])
    wt = (q._cols + 1 + 63) // 64
    jobs = []
    for s in seeds:
        terms = random_terms(random.Random(5000 + s), n, rows, 4)
        want = to_aug(expand_ints(q, *terms), q._cols, wt)
        jobs.append((f"quad_expand_words n{n} #{s}", lambda terms=terms: hip.quad_expand_words(*terms, n), want))
    return jobs


def cubic_expand_jobs(seeds, n: int = 17, rows: int = 6) -> list:
    from tests.cubic_terms import expand_ints as expand3, random_cubic_terms
    cols, jobs = xl3_cols(n), []
    for s in seeds:
        terms = random_cubic_terms(random.Random(6000 + s), n, rows)
        want = to_aug(expand3(n, *terms), cols, (cols + 1 + 63) // 64)
        jobs.append((f"cubic_expand_words n{n} #{s}", lambda terms=terms: hip.cubic_expand_words(*terms, n), want))
    return jobs


def quartic_expand_jobs(seeds, n: int = 9, rows: int = 6) -> list:
    from tests.cubic_xl4_terms import quartic_aug
    from tests.quartic_terms import expand_ints4, random_quartic_terms
    wt, jobs = (xl4_cols(n) + 1 + 63) // 64, []
    for s in seeds:
        terms = random_quartic_terms(random.Random(7000 + s), n, rows)
        want = quartic_aug(expand_ints4(n, *terms), n, rows, wt)
        jobs.append((f"quartic_expand_words n{n} #{s}", lambda terms=terms: hip.quartic_expand_words(*terms, n), want))
    return jobs


def _quad_eqs(rng, n: int, m: int) -> list:
    return expand_ints(QuadraticSystem([n]), *random_terms(rng, n, m, 4))


def xl3_expand_jobs(seeds, n: int = 33, m: int = 2) -> list:
    cols, jobs = xl3_cols(n), []
    rows, stride = m * (n + 1), (cols + 1 + 63) // 64
    for s in seeds:
        eqs = _quad_eqs(random.Random(8000 + s), n, m)
        quad = X.quad_aug(eqs, n)
        want = O.eqs_to_aug(X.xl3_ints(eqs, n), cols, stride)
        jobs.append((f"xl3_expand_words n{n} #{s}", lambda quad=quad: hip.xl3_expand_words(quad, n, rows=rows, stride_words=stride), want))
    return jobs


def xl4_expand_jobs(seeds, n: int = 13, m: int = 2) -> list:
    rows, stride, jobs = m * X4.rows_per_equation(n), (xl4_cols(n) + 1 + 63) // 64, []
    for s in seeds:
        eqs = _quad_eqs(random.Random(9000 + s), n, m)
        quad = X.quad_aug(eqs, n)
        want = X4.xl4_aug(eqs, n, rows, stride)
        jobs.append((f"xl4_expand_words n{n} #{s}", lambda quad=quad: hip.xl4_expand_words(quad, n, rows=rows, stride_words=stride), want))
    return jobs


def xl4_cubic_expand_jobs(seeds, n: int = 1) -> list:
    """n = 1: the smallest n of tests/test_gpu_cubic_xl4.py (no pair, triple or quadruple block)"""
    from tests.cubic_terms import poly_int, random_cubic_terms, row_polys
    from tests.cubic_xl4_terms import quartic_aug, xl4_cubic_eqs
    cols3, wt, jobs = xl3_cols(n), (xl4_cols(n) + 1 + 63) // 64, []
    for s in seeds:
        polys = row_polys(n, *random_cubic_terms(random.Random(10000 + s), n, 3))
        src = to_aug([poly_int(p, n) for p in polys], cols3, (cols3 + 1 + 63) // 64 + 1)
        rows, stride = len(polys) * (n + 1) + 3, wt + 2 + (wt & 1)
        want = quartic_aug(xl4_cubic_eqs(n, polys), n, rows, stride)
        jobs.append((f"xl4_cubic_expand_words n{n} #{s}", lambda src=src, rows=rows, stride=stride: hip.xl4_cubic_expand_words(src, n, rows=rows, stride_words=stride), want))
    return jobs


def specialise_jobs(seeds, n: int = 12, guess: tuple = (7, 2, 3, 11, 5), m: int = 3) -> list:
    """hip.quad_specialise_words: every assignment of five scattered unknowns (a case of _specialise_cases at n = 12)"""
    cols2, na, jobs = n + n * (n - 1) // 2, 1 << len(guess), []
    for s in seeds:
        rng = random.Random(11000 + s)
        eqs = [rng.getrandbits(cols2 + 1) for _ in range(m)]
        quad = X.quad_aug(eqs, n)
        want = G.specialised_aug(eqs, n, guess, 0, na)
        jobs.append((f"quad_specialise_words n{n} #{s}", lambda quad=quad: hip.quad_specialise_words(quad, n, guess, 0, na), want))
    return jobs


def xl3_guess_jobs(seeds, n: int = 9, m: int = 8, guess: tuple = (1, 8), mode: int = 1) -> list:
    """hip.solve_xl3_guess_words at the smallest case of tests/xl_guess_terms.CASES: a gang batch of four systems inside"""
    jobs = []
    for s in seeds:
        rng = random.Random(12000 + s)
        eqs = X.planted_dense(rng, n, m, [rng.getrandbits(n)])
        quad = X.quad_aug(eqs, n)
        want = tuple(T.oracle_key(G.oracle_guess(eqs, n, guess, a)[mode], mode) for a in range(1 << len(guess)))
        jobs.append((f"solve_xl3_guess_words n{n} #{s}", lambda quad=quad: solve_many(hip.solve_xl3_guess_words(quad, n, guess, mode=mode), mode), want))
    return jobs


# -- the forms searches against zero sets known by construction ------------------------------------------------------------------------------
# degree: (reference module, search entry, R -> (p, s) of known_zero_case: the shapes the single-thread tests have at these R)
FORMS = {
    "quad": (QF, hip.quad_forms_search, {13: (7, 3), 18: (11, 4)}),
    "cubic": (CF, hip.cubic_forms_search, {13: (5, 1), 18: (6, 0)}),
    "quartic": (Q4F, hip.quartic_forms_search, {13: (6, 1), 18: (5, 0)}),
}


def forms_case(kind: str, R: int, seed: int) -> tuple:
    """(forms, sorted zeros): R = 13 runs one partial workgroup and is padded to 65 forms (k_forms_check crosses a wave), R = 18 the
    first whole workgroups"""
    ref, _, shapes = FORMS[kind]
    rng = random.Random(13000 + 100 * R + seed)
    forms, zeros = ref.known_zero_case(rng, R, *shapes[R], "shuffled")
    if R == 13:
        forms = pad_to(rng, forms, 65)
    return list(forms), list(zeros)


def forms_jobs(kind: str, seeds, sizes=(13, 18)) -> list:
    search, jobs = FORMS[kind][1], []
    for s in seeds:
        R = sizes[s % len(sizes)]
        forms, zeros = forms_case(kind, R, s)
        jobs.append((f"{kind}_forms_search R{R} #{s}", lambda forms=forms, R=R: search(forms, R), (len(zeros), zeros)))
    return jobs


def _rank(vecs) -> int:
    piv = {}
    for v in vecs:
        while v:
            h = v.bit_length() - 1
            if h not in piv:
                piv[h] = v
                break
            v ^= piv[h]
    return len(piv)


def plan_space(kind: str, rng, n: int = 12, r: int = 10, k: int = 3, kbits: int = 40) -> tuple:
    """(origin, basis) of projection rank r over the product columns of `kind` (the _space of the forms tests)"""
    S = {"quad": n * (n - 1) // 2, "cubic": hip.cubic_cols(n) - n, "quartic": hip.quartic_cols(n) - n}[kind]
    high = ((1 << n) - 1) >> r << r
    sparse = lambda bits: sum(1 << (n + rng.randrange(S)) for _ in range(bits))      # noqa: E731
    while True:
        if kind == "quad":
            basis = [(1 << a) | (rng.getrandbits(n) & high) | (rng.getrandbits(S) << n) for a in range(r)] + [rng.getrandbits(S) << n for _ in range(k)]
        else:
            basis = [(1 << a) | (rng.getrandbits(n) & high) | sparse(6) for a in range(r)] + [sparse(kbits) for _ in range(k)]
        if _rank(basis) == r + k:
            break
    rng.shuffle(basis)
    return rng.getrandbits(n + S), basis


def plan_jobs(kind: str, seeds, n: int = 12) -> list:
    """hip.*_plan(device=0) at (12, 10, 3, 40) against the host twin (computed here: it touches no device)"""
    plan, jobs = {"quad": hip.quad_plan, "cubic": hip.cubic_plan, "quartic": hip.quartic_plan}[kind], []
    for s in seeds:
        origin, basis = plan_space(kind, random.Random(14000 + s))
        want = plan(origin, basis, n)
        assert want["r"] == 10
        jobs.append((f"{kind}_plan device #{s}", lambda origin=origin, basis=basis: plan(origin, basis, n, device=0), want))
    return jobs


# every entry group of part (a): name -> builder(seeds)
GROUPS = {
    "solve_small": lambda seeds: solve_jobs(seeds, 66, 65, None),
    "solve_blocked": lambda seeds: solve_jobs(seeds, 2600, 2500, 2300),
    "solve_rhs": rhs_jobs,
    "solve_batch": batch_jobs,
    "space_enumerate": space_jobs,
    "quad_expand": quad_expand_jobs,
    "cubic_expand": cubic_expand_jobs,
    "quartic_expand": quartic_expand_jobs,
    "xl3_expand": xl3_expand_jobs,
    "xl4_expand": xl4_expand_jobs,
    "xl4_cubic_expand": xl4_cubic_expand_jobs,
    "quad_specialise": specialise_jobs,
    "xl3_guess": xl3_guess_jobs,
    "quad_forms_search": lambda seeds: forms_jobs("quad", seeds),
    "cubic_forms_search": lambda seeds: forms_jobs("cubic", seeds),
    "quartic_forms_search": lambda seeds: forms_jobs("quartic", seeds),
    "quad_plan": lambda seeds: plan_jobs("quad", seeds),
    "cubic_plan": lambda seeds: plan_jobs("cubic", seeds),
    "quartic_plan": lambda seeds: plan_jobs("quartic", seeds),
}


# -- the extra jobs of the mixed table ------------------------------------------------------------------------------------------------------
def list_of_int_jobs() -> list:
    """_internal.m4ri_solve on the README system, m4ri_solve_many on 5 small systems (two shares: host threads of its own)"""
    from gf2bv_amd import _internal
    readme = [15, 20, 11, 0]
    rng = random.Random(15000)
    rows, cols = 70, 64
    systems = [random_system(rng, rows, cols, .5, cap, cons, 0) for cap, cons in ((None, True), (40, True), (1, True), (50, False), (63, True))]
    want_many = tuple(T.space_key(O.m4ri_solve(list(e), cols, 1)) for e in systems)
    return [
        ("m4ri_solve README", lambda: T.space_key(_internal.m4ri_solve(list(readme), 4, 1)), T.space_key(O.m4ri_solve(list(readme), 4, 1))),
        ("m4ri_solve_many 5", lambda: tuple(T.space_key(sp) for sp in _internal.m4ri_solve_many(systems, cols, 1, [0, 0])), want_many),
    ]


def search_all_jobs() -> list:
    """search_all_quartic on the n = 12 register with 10 outputs (6 states fit) and search_all_cubic with 40 (dimension 258, the
    smallest case above the host walk; the secret alone fits), against brute force over the 4096 states"""
    from gf2bv_amd import PackedCubicSystem, PackedQuarticSystem, search_all_cubic, search_all_quartic
    from tests.cubic_terms import REGISTER_12, register_zeros
    from tests.quartic_terms import REGISTER4_12, register4_brute, register4_zeros
    from tests.test_gpu_cubic_search import _cubic_brute
    secret = 0x52F
    c4 = PackedQuarticSystem([12])
    z4 = tuple(register4_zeros(c4, secret, count=10, **REGISTER4_12))
    want4 = sorted((s,) for s in register4_brute(secret, count=10, **REGISTER4_12))
    assert len(want4) == 6 and (secret,) in want4
    c3 = PackedCubicSystem([12])
    z3 = tuple(register_zeros(c3, secret, REGISTER_12["taps"], REGISTER_12["pos"], 40))
    want3 = sorted(_cubic_brute(secret, 40))
    assert want3 == [(secret,)]
    return [
        ("search_all_quartic n12 10 outputs", lambda: sorted(search_all_quartic(c4, z4)), want4),
        ("search_all_cubic n12 40 outputs", lambda: sorted(search_all_cubic(c3, z3)), want3),
    ]


def device_pair_job(n: int = 12, live: int = 60, tail: int = 8) -> tuple:
    """quad_expand_device into a sentinel-filled buffer and solve_device on the same per-thread torch stream, no synchronisation in
    between: the oracle's answer for the expanded rows, and the sentinel words behind the matrix untouched"""
    import torch
    q = QuadraticSystem([n])
    cols = q._cols
    rows, stride = cols + 2, hip.padded_stride(cols)
    terms = random_terms(random.Random(16000), n, live, 3)
    x = 0xA5B & ((1 << n) - 1)                         # the constants chosen so that every row vanishes at the consistent point of x
    point = x | sum(1 << (n + i * (i - 1) // 2 + j) for i in range(1, n) for j in range(i) if (x >> i) & (x >> j) & 1)
    for r, e in enumerate(expand_ints(q, *terms)):
        terms[0][r, 0] ^= np.uint64(bin(e & ((point << 1) | 1)).count("1") & 1)
    aug = to_aug(expand_ints(q, *terms) + [0] * (rows - live), cols, stride)
    ref = O.solve_words(aug, rows, cols, 1)
    assert ref["status"] == 0 and 0 < ref["rank"] < cols
    want = (T.oracle_key(ref, 1), True)
    flat = [np.ascontiguousarray(a).view(np.int64).reshape(-1) for a in terms]
    local = threading.local()

    def call():
        if not hasattr(local, "stream"):
            local.stream = torch.cuda.Stream()
        st = local.stream
        with torch.cuda.stream(st):
            d = [torch.from_numpy(a).cuda() for a in flat]
            d_aug = torch.full((rows * stride + tail,), SENTINEL, dtype=torch.int64, device="cuda")
            hip.quad_expand_device(*[t.data_ptr() for t in d], live, rows, n, d_aug.data_ptr(), stride, stream=st.cuda_stream)
            sol = hip.solve_device(d_aug.data_ptr(), rows, cols, stride, 1, stream=st.cuda_stream)
            behind = d_aug[rows * stride:].cpu().numpy()
        st.synchronize()
        return T.solution_key(sol, 1), bool((behind == SENTINEL).all())
    return "quad_expand_device + solve_device", call, want


def mixed_jobs() -> list:
    """one job of every entry group and the extras"""
    jobs = [build([20 + k])[0] for k, (name, build) in enumerate(GROUPS.items()) if not name.endswith("forms_search")]
    for kind in FORMS:
        jobs += forms_jobs(kind, [20, 21])                        # (an even and an odd seed: R = 13 and R = 18)
    return jobs + list_of_int_jobs() + search_all_jobs() + [device_pair_job()]
