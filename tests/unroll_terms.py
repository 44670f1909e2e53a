"""Host twin of the unrolling entries (gf2bv_compose_unroll_*), written from their meaning: the map substituted into the watched forms
one time step after the other with tests/compose_terms.py.  No doubling, no blocks: nothing is shared with the library's schedule.
Only a start or a step too large to walk is reached through compose_terms.power, which squares least significant bit first."""
from __future__ import annotations

import numpy as np

from tests import compose_terms as T

WALK = 4096                     # exponents up to here are walked one substitution at a time


def _map_power(b: np.ndarray, n: int, k: int) -> np.ndarray:
    return T.power_loop(b, n, k) if k <= WALK else T.power(b, n, k)


def unroll(a: np.ndarray, n: int, b: np.ndarray, start: int, step: int, count: int, stride: int | None = None) -> np.ndarray:
    """[count * len(a), stride] uint64, time-major: row i * len(a) + r = a[r] with b substituted start + i * step times"""
    assert len(b) == n and start >= 0 and step >= 1 and count >= 0
    w = T.form_words(n) if stride is None else stride
    out = np.zeros((count * len(a), w), dtype=np.uint64)
    if count == 0 or len(a) == 0:
        return out
    ident = T.identity(n)
    # a o b^start: substituting the identity only drops the bits above n
    cur = T.substitute(a, n, ident if start == 0 else _map_power(b, n, start), n)
    stepped = None
    for i in range(count):
        if i:
            if step <= WALK:
                for _ in range(step):
                    cur = T.substitute(cur, n, b, n)
            else:
                if stepped is None:
                    stepped = T.power(b, n, step)
                cur = T.substitute(cur, n, stepped, n)
        out[i * len(a):(i + 1) * len(a), :T.form_words(n)] = cur
    return out


def _pw(k: int) -> int:
    return k.bit_length() - 1 + bin(k).count("1") if k else 0


def products(start: int, step: int, count: int) -> int:
    """the product count of the library's fixed schedule, from its formula"""
    doubling = 2 * (count - 1).bit_length() - 1 if count >= 2 else 0          # (count - 1).bit_length() = ceil(log2 count)
    return (_pw(step) if step > 1 else 0) + (_pw(start) + 1 if start > 0 else 0) + doubling
