"""The library's environment switches as it parses them (gf2bv_knob_dump through hip.knobs(); no GPU).

One table in gf2_solver.hip (Knobs) reads every GF2BV_* variable of libgf2bv_hip.so; DESIGN.md, "Environment switches", is its
documentation.  Every row of that section is checked here with at least one in-range value, one out-of-range value and, where
the row tells them apart, the empty text.
"""
import os
import re

import pytest

from gf2bv_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = {
    "GF2BV_PLAIN": "0", "GF2BV_STREAM_PAIRS": "unset", "GF2BV_UPDATE": "0", "GF2BV_TWO_LEVEL": "unset",
    "GF2BV_TWO_LEVEL_MIN_MIB": "unset", "GF2BV_OUTER_CHAIN": "0", "GF2BV_OUTER_SIDE": "1", "GF2BV_FAST": "1",
    "GF2BV_OPTIMISTIC": "unset", "GF2BV_FUSED_NARROW": "1", "GF2BV_SPARSE_FAST": "1", "GF2BV_PC": "1", "GF2BV_FLAG_SYNC": "1",
    "GF2BV_SERIAL": "0", "GF2BV_XCD_PIN": "unset", "GF2BV_XCD_WGS": "32", "GF2BV_GANG_NT": "1", "GF2BV_GANG_BS": "1",
    "GF2BV_BS_INV": "unset", "GF2BV_YSWEEP": "0", "GF2BV_SMALL": "1", "GF2BV_SMALL_ZC": "unset", "GF2BV_SELF_WAIT_US": "50",
    "GF2BV_GANG": "0", "GF2BV_BATCH_THREADS": "2", "GF2BV_SLAB_PAD": "64", "GF2BV_KEEP_BIG": "1", "GF2BV_HOST_POOL_MB": "4608",
    "GF2BV_TRACE": "0", "GF2BV_DEBUG_SYNC": "0", "GF2BV_SMALL_PROBE": "0",
}


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("GF2BV_") and name != "GF2BV_LIB":
            monkeypatch.delenv(name)
    return monkeypatch


def test_defaults(clean_env):
    assert hip.knobs() == DEFAULTS
    assert len(DEFAULTS) == 31


# (variable, text, what the dump says then): in range, out of range, and the empty text where the row distinguishes it
def _rows():
    rows = []
    # on iff set, whatever the value
    for name in ("GF2BV_TRACE", "GF2BV_SERIAL", "GF2BV_YSWEEP", "GF2BV_SMALL_PROBE"):
        rows += [(name, "1", "1"), (name, "0", "1"), (name, "", "1"), (name, "no", "1")]
    # set (empty included): atoi(e) != 0; default on
    for name in ("GF2BV_FAST", "GF2BV_FUSED_NARROW", "GF2BV_SPARSE_FAST", "GF2BV_PC", "GF2BV_GANG_NT", "GF2BV_GANG_BS"):
        rows += [(name, "0", "0"), (name, "1", "1"), (name, "7", "1"), (name, "-3", "1"), (name, "", "0"), (name, "x", "0")]
    # set: atoi(e) != 0; unset is a state of its own
    for name in ("GF2BV_STREAM_PAIRS", "GF2BV_OPTIMISTIC", "GF2BV_XCD_PIN", "GF2BV_BS_INV", "GF2BV_SMALL_ZC"):
        rows += [(name, "0", "0"), (name, "1", "1"), (name, "-2", "1"), (name, "", "0"), (name, "junk", "0")]
    rows += [
        ("GF2BV_PLAIN", "1", "1"), ("GF2BV_PLAIN", "0", "0"), ("GF2BV_PLAIN", "-1", "1"), ("GF2BV_PLAIN", "", "0"), ("GF2BV_PLAIN", "yes", "0"),
        ("GF2BV_SLAB_PAD", "2", "2"), ("GF2BV_SLAB_PAD", "1024", "1024"), ("GF2BV_SLAB_PAD", "0", "1"), ("GF2BV_SLAB_PAD", "-5", "1"),
        ("GF2BV_SLAB_PAD", "", "1"),
        ("GF2BV_KEEP_BIG", "0", "0"), ("GF2BV_KEEP_BIG", "1", "1"), ("GF2BV_KEEP_BIG", "-1", "1"), ("GF2BV_KEEP_BIG", "", "0"),
        ("GF2BV_HOST_POOL_MB", "0", "0"), ("GF2BV_HOST_POOL_MB", "100", "100"), ("GF2BV_HOST_POOL_MB", "-1", "4608"),
        ("GF2BV_HOST_POOL_MB", "", "0"),
        ("GF2BV_UPDATE", "0", "0"), ("GF2BV_UPDATE", "5", "5"), ("GF2BV_UPDATE", "6", "0"), ("GF2BV_UPDATE", "-1", "0"), ("GF2BV_UPDATE", "", "0"),
        ("GF2BV_TWO_LEVEL", "0", "0"), ("GF2BV_TWO_LEVEL", "-4", "0"), ("GF2BV_TWO_LEVEL", "1", "2"), ("GF2BV_TWO_LEVEL", "2", "2"),
        ("GF2BV_TWO_LEVEL", "8", "8"), ("GF2BV_TWO_LEVEL", "12", "12"), ("GF2BV_TWO_LEVEL", "99", "12"), ("GF2BV_TWO_LEVEL", "", "unset"),
        ("GF2BV_TWO_LEVEL", "k", "0"),
        ("GF2BV_TWO_LEVEL_MIN_MIB", "384", "384"), ("GF2BV_TWO_LEVEL_MIN_MIB", "0.5", "0.5"), ("GF2BV_TWO_LEVEL_MIN_MIB", "0", "0"),
        ("GF2BV_TWO_LEVEL_MIN_MIB", "-1", "-1"), ("GF2BV_TWO_LEVEL_MIN_MIB", "", "unset"),
        ("GF2BV_OUTER_CHAIN", "1", "1"), ("GF2BV_OUTER_CHAIN", "0", "0"), ("GF2BV_OUTER_CHAIN", "5", "1"), ("GF2BV_OUTER_CHAIN", "", "0"),
        ("GF2BV_OUTER_SIDE", "0", "0"), ("GF2BV_OUTER_SIDE", "1", "1"), ("GF2BV_OUTER_SIDE", "-1", "1"), ("GF2BV_OUTER_SIDE", "", "1"),
        ("GF2BV_DEBUG_SYNC", "1", "1"), ("GF2BV_DEBUG_SYNC", "2", "2"), ("GF2BV_DEBUG_SYNC", "3", "3"), ("GF2BV_DEBUG_SYNC", "", "0"),
        ("GF2BV_DEBUG_SYNC", "q", "0"),
        ("GF2BV_FLAG_SYNC", "0", "0"), ("GF2BV_FLAG_SYNC", "1", "1"), ("GF2BV_FLAG_SYNC", "2", "2"), ("GF2BV_FLAG_SYNC", "", "0"),
        ("GF2BV_FLAG_SYNC", "9", "9"),
        ("GF2BV_XCD_WGS", "16", "16"), ("GF2BV_XCD_WGS", "256", "256"), ("GF2BV_XCD_WGS", "0", "1"), ("GF2BV_XCD_WGS", "1000", "256"),
        ("GF2BV_XCD_WGS", "-8", "1"), ("GF2BV_XCD_WGS", "", "1"),
        ("GF2BV_SELF_WAIT_US", "0", "0"), ("GF2BV_SELF_WAIT_US", "5", "5"), ("GF2BV_SELF_WAIT_US", "1000000", "1000000"),
        ("GF2BV_SELF_WAIT_US", "1000001", "50"), ("GF2BV_SELF_WAIT_US", "-1", "50"), ("GF2BV_SELF_WAIT_US", "", "0"),
        ("GF2BV_GANG", "1", "1"), ("GF2BV_GANG", "24", "24"), ("GF2BV_GANG", "0", "0"), ("GF2BV_GANG", "-3", "0"), ("GF2BV_GANG", "", "0"),
        ("GF2BV_BATCH_THREADS", "1", "1"), ("GF2BV_BATCH_THREADS", "16", "16"), ("GF2BV_BATCH_THREADS", "64", "16"),
        ("GF2BV_BATCH_THREADS", "0", "2"), ("GF2BV_BATCH_THREADS", "-1", "2"), ("GF2BV_BATCH_THREADS", "", "2"),
        ("GF2BV_SMALL", "0", "0"), ("GF2BV_SMALL", "1", "1"), ("GF2BV_SMALL", "-1", "1"), ("GF2BV_SMALL", "", "0"),
    ]
    return rows


@pytest.mark.parametrize("name,text,want", _rows())
def test_row(clean_env, name, text, want):
    clean_env.setenv(name, text)
    got = hip.knobs()
    assert got[name] == want
    assert {k: v for k, v in got.items() if k != name} == {k: v for k, v in DEFAULTS.items() if k != name}   # nothing else moves


def test_every_variable_has_rows():
    assert {r[0] for r in _rows()} == set(DEFAULTS)


# GF2BV_PLAIN changes the DEFAULT of four heuristics and nothing in the table: the three switches that win over it stay "unset" until
# they are set, and then hold what was asked for whatever plain says.  (What a solve makes of the pair -- explicit value if set, else
# !plain -- is one block of solver_alloc and one line of Pool::low_stream_for; the GPU parity files run under both.)
WIN_OVER_PLAIN = ("GF2BV_STREAM_PAIRS", "GF2BV_XCD_PIN", "GF2BV_OPTIMISTIC")


def test_plain_alone(clean_env):
    clean_env.setenv("GF2BV_PLAIN", "1")
    k = hip.knobs()
    assert k == {**DEFAULTS, "GF2BV_PLAIN": "1"}
    assert all(k[name] == "unset" for name in WIN_OVER_PLAIN)


@pytest.mark.parametrize("name", WIN_OVER_PLAIN)
@pytest.mark.parametrize("text", ["1", "0"])
def test_explicit_switch_beside_plain(clean_env, name, text):
    clean_env.setenv("GF2BV_PLAIN", "1")
    clean_env.setenv(name, text)
    assert hip.knobs() == {**DEFAULTS, "GF2BV_PLAIN": "1", name: text}
    clean_env.setenv("GF2BV_PLAIN", "0")
    assert hip.knobs() == {**DEFAULTS, name: text}


def test_change_between_two_dumps_is_seen(clean_env):
    assert hip.knobs()["GF2BV_GANG"] == "0"
    clean_env.setenv("GF2BV_GANG", "8")
    assert hip.knobs()["GF2BV_GANG"] == "8"
    clean_env.setenv("GF2BV_GANG", "16")
    assert hip.knobs()["GF2BV_GANG"] == "16"
    clean_env.delenv("GF2BV_GANG")
    assert hip.knobs()["GF2BV_GANG"] == "0"
    # the process-lifetime switches too: the dump parses, it does not latch
    clean_env.setenv("GF2BV_SLAB_PAD", "2")
    assert hip.knobs()["GF2BV_SLAB_PAD"] == "2"
    clean_env.setenv("GF2BV_SLAB_PAD", "128")
    assert hip.knobs()["GF2BV_SLAB_PAD"] == "128"


def test_dump_buffer_too_small():
    import ctypes
    buf = ctypes.create_string_buffer(16)
    assert hip.lib().gf2bv_knob_dump(buf, len(buf)) == 1           # GF2BV_ERR_ARG
    assert hip.lib().gf2bv_knob_dump(None, 4096) == 1


def _solver_source():
    with open(os.path.join(ROOT, "gf2bv_amd", "csrc", "gf2_solver.hip")) as f:
        return f.read()


def _function_body(src, head):
    """the text of the braces that follow `head`"""
    at = src.index(head)
    start = src.index("{", at)
    depth = 0
    for i in range(start, len(src)):
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        if depth == 0:
            return start, i + 1
    raise AssertionError("unbalanced braces")


def test_getenv_only_in_the_reader():
    src = _solver_source()
    lo, hi = _function_body(src, "static Knobs read(")
    calls = [m.start() for m in re.finditer(r"getenv", src)]             # (comments included)
    assert calls and all(lo <= at < hi for at in calls)
    # one call per variable, and the dump prints the same names
    named = re.findall(r'getenv\("(GF2BV_[A-Z_]+)"\)', src[lo:hi])
    assert len(named) == len(calls) and sorted(named) == sorted(DEFAULTS)
    for gone in ("ext_events", "sparse_mode", "fused_rpt", "plain_mode"):
        assert gone not in src, gone


def test_design_section_lists_what_the_dump_prints():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        doc = f.read()
    at = doc.index("## 8. Environment switches")
    section = doc[at:doc.index("\n## ", at + 1)]
    table = [line for line in section.splitlines() if line.startswith("| `GF2BV_")]
    listed = [re.match(r"\| `(GF2BV_[A-Z_]+)`", line).group(1) for line in table]
    assert sorted(listed) == sorted(hip.knobs())
    # the variables of the other binaries are named below the table, not in it
    for other in ("GF2BV_DEVICE", "GF2BV_BATCH_CHUNK_MB", "GF2BV_LIB"):
        assert other in section and other not in listed
