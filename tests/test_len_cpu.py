"""ks_len.h: floor(a / eps) from a reciprocal, against Python's exact a // eps.

The header is compiled for the host (tests/len_host.cpp, g++) with the same double
arithmetic the device runs: a multiply and a floor, both correctly rounded, no
contraction possible. Inputs are the function's whole contract, |a| < 2^62 and
eps >= 1 (include/ksmcmf.h): the edge multiples k·eps − 1, k·eps, k·eps + 1 around
the 2^41 estimate limit are kept wherever they lie inside that range (for eps 2^45
and 2^60 the multiples of ±2^41 are beyond 64 bits: no long long holds them)."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = [1, 2, 3, 121253, 2**20 - 1, 2**20 + 1, 2**45, 2**60]
KS = [0] + [s * k for k in (1, 2**41 - 1, 2**41, 2**41 + 1) for s in (1, -1)]
LIM = 2**62


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("len") / "len_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "len_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.len_floordiv.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    L.len_floordiv.restype = None
    L.len_fallbacks.restype = ctypes.c_longlong
    return L


def run(L, pairs):
    """(quotients, calls that took the division) for [(a, eps)]."""
    n = len(pairs)
    A = (ctypes.c_longlong * n)(*[a for a, _ in pairs])
    E = (ctypes.c_longlong * n)(*[e for _, e in pairs])
    Q = (ctypes.c_longlong * n)()
    L.len_reset()
    L.len_floordiv(A, E, Q, n)
    return list(Q), L.len_fallbacks()


def edge_pairs():
    out = []
    for e in EPS:
        vals = {0, 1, -1, LIM - 1, -(LIM - 1)}
        for k in KS:
            vals.update((k * e - 1, k * e, k * e + 1))
        out += [(a, e) for a in sorted(vals) if abs(a) < LIM]
    return out


def test_edges_equal_exact_division(lib):
    pairs = edge_pairs()
    # the cases the 2^41 limit is about are present on both sides of it
    assert (2**41 * 3, 3) in pairs and ((2**41 - 1) * 3 + 1, 3) in pairs and (-(2**41 + 1) * 121253 - 1, 121253) in pairs
    got, fb = run(lib, pairs)
    bad = [(a, e, q, a // e) for (a, e), q in zip(pairs, got) if q != a // e]
    assert not bad, bad[:10]
    assert 0 < fb < len(pairs), f"division taken by {fb} of {len(pairs)} calls"


def test_each_side_of_the_limit(lib):
    """k·eps − 1 … k·eps + 1: |k| = 2^41 − 1 stays on the multiply (k·eps + 1 at the
    top rounds to 2^41 − 1 + 1/eps < 2^41 for eps > 1), |k| = 2^41 + 1 takes the division."""
    for e in (2, 3, 121253, 2**20 - 1, 2**20 + 1):
        below = [(s * (2**41 - 1) * e + d, e) for s in (1, -1) for d in (-1, 0, 1)]
        above = [(s * (2**41 + 1) * e + d, e) for s in (1, -1) for d in (-1, 0, 1)]
        got, fb = run(lib, below)
        assert got == [a // e for a, e in below] and fb == 0, (e, fb)
        got, fb = run(lib, above)
        assert got == [a // e for a, e in above] and fb == len(above), (e, fb)


def test_random_pairs(lib):
    rng = random.Random(20250611)
    pairs = []
    for i in range(10**6):
        a = rng.randrange(-(LIM - 1), LIM)
        if i % 4 == 0:
            a >>= rng.randrange(0, 62)   # every magnitude, not only the top bits
        e = EPS[i % len(EPS)] if i % 2 else max(1, rng.randrange(1, 2**60) >> rng.randrange(0, 60))
        if i % 8 == 0:   # near a multiple of eps, the quotient in reach of the multiply
            a = (rng.randrange(-2**41, 2**41) * e + rng.randrange(-2, 3))
            if abs(a) >= LIM:
                a = rng.randrange(-2, 3)
        pairs.append((a, e))
    got, fb = run(lib, pairs)
    bad = [(a, e, q, a // e) for (a, e), q in zip(pairs, got) if q != a // e]
    assert not bad, bad[:10]
    assert 0 < fb < len(pairs), f"division taken by {fb} of {len(pairs)} calls"
