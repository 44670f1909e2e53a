"""The packed quadratic front-end on the MI355X: factored equations expanded into the linearised matrix on the device (k_quad_expand)
and solved there.  The yardstick throughout is the int front-end -- QuadraticSystem and mul_bit_quad on the host -- on the same
equations; every comparison is bit-exact."""
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedQuadBitVec, PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError
from gf2bv_amd.packed import _popcount64
from tests.harness_models import FibonacciLFSR, GaloisLFSR
from tests.quad_terms import expand_ints, random_terms, to_aug
from tests.test_gpu_quad_search import N_BITS, SELECT, TAPS, _filter, _raw
from tests.test_gpu_stream_order import _delayed_copy, _handle, cycles, stream      # noqa: F401  (fixtures)


@pytest.fixture(params=["default", "plain"])
def mode(request, monkeypatch):
    """every test as shipped and with GF2BV_PLAIN=1 (the solves underneath on their plain paths)"""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


# (the timeout: the n = 256 case expands and solves a 32960 x 32896 system twice and multiplies 128 products of 256-bit forms on the host)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900), pytest.mark.usefixtures("mode")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


# -- 4. expansion parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 128, 190])
def test_expansion_equals_int_front_end(n):
    rng = random.Random(4000 + n)
    q = QuadraticSystem([n])
    wt = (q._cols + 1 + 63) // 64
    for live, rows, stride, max_terms in ((13, 13, wt, 4), (9, 14, wt + 3, 4), (3, 5, wt + (wt & 1), 11), (0, 2, wt, 0)):
        lin, off, ta, tb = random_terms(rng, n, live, max_terms)          # (11: more products than one pass of the kernel holds)
        got = hip.quad_expand_words(lin, off, ta, tb, n, rows=rows, stride_words=stride)
        want = to_aug(expand_ints(q, lin, off, ta, tb) + [0] * (rows - live), q._cols, stride)
        assert got.shape == want.shape == (rows, stride)
        assert np.array_equal(got, want), (n, live, rows, stride, np.argwhere(got != want)[:4])      # every word of the stride
    assert hip.quad_expand_words(lin, off, ta, tb, n, rows=0).shape == (0, wt)


# -- 5. solve parity on rank-deficient systems -----------------------------------------------------------------------------------------
def _planted_twin(rng, n: int, neq: int, secrets: int):
    """test_gpu_quad_search._planted on both front-ends in step: random quadratic equations that vanish at `secrets` points"""
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    (x,), (y,) = q.gens(), p.gens()
    raws = [_raw(n, rng.getrandbits(n)) for _ in range(secrets)]
    zq, zp = [], []
    while len(zq) < neq:
        k = rng.randrange(n)
        e, f = x[k], y[k]
        for _ in range(rng.randint(1, 3)):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b:
                e, f = e ^ q.mul_bit(x[a], x[b]), f ^ p.mul_bit(y[a], y[b])
        vals = {e.evaluate(r) for r in raws}
        if len(vals) == 1:
            v = vals.pop()
            zq.append(e ^ v)
            zp.append(f ^ v)
    return q, p, zq, zp


def _space(sp):
    return None if sp is None else (sp.dimension, sp.origin, sp.basis)


def test_solves_equal_int_front_end():
    rng = random.Random(7)
    seen_multi = seen_high = seen_large = seen_padded = 0
    for trial in range(18):
        n = rng.randint(6, 24)
        cols = n + n * (n - 1) // 2
        neq = rng.randint(max(1, cols - 16), cols + 8) if trial else cols - 30        # (trial 0: beyond solve_all's default limit)
        q, p, zq, zp = _planted_twin(rng, n, neq, secrets=1 + (trial % 3))
        sq, sp = q.solve_raw_space(zq), p.solve_raw_space(zp)
        assert _space(sp) == _space(sq) and sq is not None, (n, neq)
        assert p.solve_raw_one(zp) == q.solve_raw_one(zq)
        seen_padded += neq < cols
        d = sq.dimension
        if d > 16:
            with pytest.raises(DimensionTooLargeError) as eq:
                list(q.solve_all(zq))
            with pytest.raises(DimensionTooLargeError) as ep:
                list(p.solve_all(zp))
            assert _space(ep.value.space) == _space(eq.value.space) == _space(sq)
            with pytest.raises(DimensionTooLargeError):
                p.solve_one(zp)
            seen_large += 1
        else:
            want = list(q.solve_all(zq))
            assert list(p.solve_all(zp)) == want, (n, neq, d)
            assert p.solve_one(zp) == q.solve_one(zq) == (want[0] if want else None)
            seen_multi += len(want) > 1
            seen_high += d >= 8
        assert p.search_all(zp) == q.search_all(zq), (n, neq, d)
        assert p.search_one(zp) == q.search_one(zq)
    assert seen_multi and seen_high and seen_large and seen_padded, (seen_multi, seen_high, seen_large, seen_padded)


# -- 6. what the host no longer decides: rows that expand to 0 or to the constant 1 ------------------------------------------------------
def test_rows_that_expand_to_zero_or_one():
    n = 5
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    (x,) = p.gens()
    nothing = p.mul_bit(x[0], x[1]) ^ p.mul_bit(x[1], x[0])               # expands to 0: solves as the empty system does
    assert isinstance(nothing, PackedQuadBitVec) and p.get_eqs([nothing]) == [] and p.get_eqs([]) == []
    want = q.solve_raw_space([])
    assert want.dimension == q._cols
    for zeros in ([nothing], [], [nothing, 0, nothing]):
        assert _space(p.solve_raw_space(zeros)) == _space(want)
        assert p.solve_raw_one(zeros) == q.solve_raw_one([]) == 0
        assert list(p.solve_all(zeros, max_dimension=q._cols)) == list(q.solve_all([], max_dimension=q._cols))
        assert p.search_all(zeros) == q.search_all([]) and len(p.search_all(zeros)) == 1 << n
        assert p.search_one(zeros) == q.search_one([]) == (0,)
    one = p.mul_bit(x[0], x[0]) ^ x[0] ^ 1                                # x0 x0 = x0: expands to the constant 1, "1 = 0"
    assert p.get_eqs([one]) == [1]
    for zeros in ([nothing, one], [one], [x[2] ^ x[3], one, nothing], [1], [nothing, 1]):
        assert p.solve_raw_one(zeros) is None and p.solve_raw_space(zeros) is None
        assert list(p.solve_all(zeros)) == [] and p.solve_one(zeros) is None
        assert p.search_all(zeros) == [] and p.search_one(zeros) is None


# -- 7. the filtered LFSR of examples/nlfsr_recovery.py ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [(GaloisLFSR, 1), (FibonacciLFSR, 2)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_nlfsr_recovery(kind, seed):
    secret = random.Random(seed).getrandbits(N_BITS)
    reg, out = kind(N_BITS, TAPS, secret), []
    for _ in range(2 ** 14 + 1000):
        reg()
        out.append(_filter(*[(reg.state >> i) & 1 for i in SELECT]))
    p, q = PackedQuadraticSystem([N_BITS]), QuadraticSystem([N_BITS])
    sym, ref = kind(N_BITS, TAPS, p.gens()[0]), kind(N_BITS, TAPS, q.gens()[0])
    zeros, first = [], []
    for bit in out:
        sym()
        if len(first) < 200:
            ref()
        if bit:                                       # the annihilator g = x0 x1 + x0 + x1 x2 + x1 + x2 + 1 vanishes
            x0, x1, x2 = [sym.state[i] for i in SELECT[:3]]
            zeros.append(p.mul_bit(x0, x1) ^ x0 ^ p.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
            if len(first) < 200:
                x0, x1, x2 = [ref.state[i] for i in SELECT[:3]]
                first.append(q.mul_bit(x0, x1) ^ x0 ^ q.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
    assert p.get_eqs(zeros[:200]) == q.get_eqs(first) and len(first) == 200
    assert list(p.solve_all(zeros)) == [(secret,)]
    assert p.solve_one(zeros) == (secret,)
    assert p.search_one(zeros) == (secret,)


# -- 8. a size the int front-end cannot reach --------------------------------------------------------------------------------------------
def _dense_forms(rng, count: int, n: int, constant_free: bool) -> np.ndarray:
    wl = (n + 1 + 63) // 64
    f = rng.integers(0, 1 << 64, size=(count, wl), dtype=np.uint64)
    top = (n + 1) & 63
    if top:
        f[:, -1] &= np.uint64((1 << top) - 1)
    if constant_free:
        f[:, 0] &= np.uint64(~1 & (2 ** 64 - 1))
    return f


def test_n256_planted_secret():
    """n = 256: 32896 columns, 32960 equations of two products of dense forms plus a dense linear form each -- about 700 s of
    mul_bit on the int front-end -- with constants that make a planted 256-bit secret a solution"""
    n, rows = 256, 32960
    rng = np.random.default_rng(20261016)
    lin, ta, tb = _dense_forms(rng, rows, n, True), _dense_forms(rng, 2 * rows, n, True), _dense_forms(rng, 2 * rows, n, True)
    off = np.arange(0, 2 * rows + 1, 2, dtype=np.int64)
    secret = int.from_bytes(rng.bytes(n // 8), "little")
    point = np.frombuffer((secret << 1).to_bytes(8 * lin.shape[1], "little"), dtype=np.uint64)
    par = lambda f: (_popcount64(f & point[None, :]).sum(axis=1) & 1).astype(np.uint64)          # noqa: E731  (f . x of constant-free forms)
    prod = par(ta) & par(tb)
    lin[:, 0] |= par(lin) ^ prod[0::2] ^ prod[1::2]                        # lin . x ^ sum (a . x)(b . x) ^ constant = 0
    p = PackedQuadraticSystem([n])
    zeros = [PackedQuadBitVec(lin, off, ta, tb, n)]
    space = p.solve_raw_space(zeros)
    assert space is not None and space.dimension <= 16, space and space.dimension        # (a degenerate generator must not pass unnoticed)
    assert p.search_one(zeros) == (secret,)
    aug = hip.quad_expand_words(lin, off, ta, tb, n)
    q = QuadraticSystem([n])
    pick = sorted(random.Random(8).sample(range(rows), 64))
    want = to_aug(expand_ints(q, lin[pick], np.arange(0, 129, 2), ta.reshape(rows, -1)[pick].reshape(128, -1),
                              tb.reshape(rows, -1)[pick].reshape(128, -1)), q._cols, aug.shape[1])
    assert np.array_equal(aug[pick], want)


# -- 9. stream order -----------------------------------------------------------------------------------------------------------------------
def _vanishing_at(terms, n: int, x: int):
    """the factored rows with their constants chosen so that every row vanishes at the consistent point of linear part x"""
    lin, off, ta, tb = terms
    point = (_raw(n, x & ((1 << n) - 1)) << 1) | 1
    lin = lin.copy()
    for r, e in enumerate(expand_ints(QuadraticSystem([n]), lin, off, ta, tb)):
        lin[r, 0] ^= np.uint64(bin(e & point).count("1") & 1)
    return lin, off, ta, tb


def test_expand_device_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device inputs first hold the operands of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then the expansion and the solve are enqueued there with no synchronisation anywhere."""
    n, live = 46, 900
    cols = hip.quad_cols(n)                            # 1081 columns: beyond the one-launch small path, the blocked path
    rows, stride = cols + 12, hip.padded_stride(cols)
    new, old = random_terms(random.Random(91), n, live, 3), random_terms(random.Random(92), n, live, 3)
    off = new[1]
    old = (old[0], off, np.resize(old[2], new[2].shape), np.resize(old[3], new[3].shape))          # the same products per row
    new, old = _vanishing_at(new, n, 0x2F00D5EED5A1), _vanishing_at(old, n, 0x1BADC0FFEE42)  # consistent systems: origins and bases to compare
    want, stale = hip.solve_quad_terms(*new, n, rows, 1), hip.solve_quad_terms(*old, n, rows, 1)
    assert want.status == stale.status == 0 and 0 < want.rank < cols
    key = lambda s: (s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())     # noqa: E731
    assert key(want) != key(stale), "the two systems have the same answer"
    pack = lambda t: np.concatenate([t[0].ravel(), t[2].ravel(), t[3].ravel()])                    # noqa: E731
    to_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()                                   # noqa: E731
    buf, src, d_off = to_dev(pack(old)), to_dev(pack(new)), torch.from_numpy(off).cuda()
    d_aug = torch.zeros(rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d_lin = buf.data_ptr()
    d_ta = d_lin + new[0].nbytes
    d_tb = d_ta + new[2].nbytes
    _delayed_copy(stream, cycles, buf, src)
    hip.quad_expand_device(d_lin, d_off.data_ptr(), d_ta, d_tb, live, rows, n, d_aug.data_ptr(), stride, stream=_handle(stream))
    got = hip.solve_device(d_aug.data_ptr(), rows, cols, stride, 1, stream=_handle(stream))
    assert got.stats["small_path"] == 0
    assert key(got) == key(want)
