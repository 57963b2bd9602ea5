"""The row-span layout of the upper rounds' blocks, checked on the CPU (no GPU): the layout the
device builds is exported per block and direction (cpk.rowspan_layouts) and the level loop is
replayed in numpy -- the leads folded, then per step the broadcast value, every row's masked span
read, and the drains at the table's steps -- against the plain in-order row sums of the same
entries.  Every row must come out bit for bit: same terms, same order, product and subtraction
rounded separately.  Gaps of the image hold NaN in the replay, so a gap that reached a result
would show."""
import numpy as np
import pytest

import cpkrylov_amd as cpk
import structures
from cpkrylov_amd.synthetic import saddle_system

GUARD, END_GUARD = 4, 8  # kRowspanGuard, kRowspanEndGuard (dev.hpp)
_CACHE = {}


def _layouts(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        S = saddle_system(N=60000, window=64, seed=5) if name == "w64" else structures.get(name)
        _CACHE[key] = cpk.rowspan_layouts(S["G"], S["B"], -S["C"], **kw)
    return _CACHE[key]


def _bit(mask_row, t):
    return (int(mask_row[t >> 6]) >> (t & 63)) & 1


def _replay(r, rng):
    nr, r0, rowptr, col, val, dest, step = r["nr"], r["r0"], r["rowptr"], r["col"], r["val"], r["dest"], r["step"]
    inblk = (col >= r0) & (col < r0 + nr)
    w = rng.standard_normal(int(col.max()) + 1 if len(col) else 1)  # the finished rows outside the block
    win = rng.standard_normal(nr)
    rowof = np.empty(nr, np.int64)
    rowof[step] = np.arange(nr)
    assert sorted(step.tolist()) == list(range(nr))
    # the plain sums: rows in step order, every row's entries in their stored order
    ref = win.copy()
    for t in range(nr):
        k = rowof[t]
        acc = ref[k]
        for e in range(rowptr[k], rowptr[k + 1]):
            x = ref[col[e] - r0] if inblk[e] else w[col[e]]
            acc = acc - val[e] * x
        ref[k] = acc
    # the image
    slots = r["slots"]
    assert len(set(dest.tolist())) == len(dest) and (dest.min(initial=slots - 1) >= GUARD) and dest.max(initial=0) < slots - END_GUARD
    img = np.full(slots, np.nan)
    img[dest] = np.where(inblk, val, val * w[col])
    acc = win.copy()
    for k in range(nr):  # the fold: the leading outside products, in order
        e = rowptr[k]
        n = 0
        while e + n < rowptr[k + 1] and not inblk[e + n]:
            n += 1
        assert np.array_equal(dest[e:e + n], r["lead"][k] + np.arange(n))
        for j in range(n):
            acc[k] = acc[k] - img[r["lead"][k] + j]
    mask, base, first, run0, tab = r["mask"], r["base"], r["first"], r["run0"].copy(), r["tab"]
    s_all = np.arange(nr)
    # every group read of the level loop stays inside the image
    assert np.all(base - 3 >= 0) and np.all(base + (s_all - first) + 3 < slots) and np.all(first <= s_all)
    a = acc[rowof]  # by step
    di = 0
    for t in range(nr):
        x = a[t]
        has = np.array([_bit(mask[s], t) for s in range(nr)], bool)
        assert not np.any(has[:t + 1]), "a term at or past the row's own step"
        slot = base + (t - first)
        assert np.all((slot[has] >= base[has]) & (slot[has] < base[has] + (s_all - first)[has]))
        p = np.where(has, img[np.clip(slot, 0, slots - 1)] * x, 0.0)
        a = a - p
        if (r["dset"][t >> 6] >> (t & 63)) & 1:
            k = tab[di].astype(np.int64)
            assert np.all(k[nr:] == 0) and np.all(k[:nr][~has] == 0) and k.max() > 0
            for s in np.nonzero(k[:nr])[0]:
                assert run0[s] + k[s] + END_GUARD - 1 < slots
                for j in range(k[s]):
                    a[s] = a[s] - img[run0[s] + j]
                run0[s] += k[s]
            di += 1
    assert di == r["ndr"]
    out = np.empty(nr)
    out[rowof] = a
    assert not np.any(np.isnan(out))
    assert np.array_equal(out, ref), np.max(np.abs(out - ref))


@pytest.mark.parametrize("name", ["w64"] + sorted(structures.MEMBERS))
def test_rowspan_layout_replays_the_row_sums(name):
    rng = np.random.default_rng(61)
    for r in _layouts(name):
        if r["nr"] > 128:
            assert not r["eligible"]
        if r["eligible"]:
            _replay(r, rng)


def test_rowspan_w64_cases_and_refusals():
    """The 60 000-dof +-64 system holds the cases: one and two rows per lane, forward runs, none
    backward, and blocks of more than 128 rows, which are refused; with a small image every block
    over its capacity is refused."""
    L = _layouts("w64")
    el = [r for r in L if r["eligible"]]
    assert any(r["nr"] > 64 for r in el) and any(r["nr"] <= 64 for r in el)
    assert any(r["nr"] > 128 for r in L) and not any(r["eligible"] for r in L if r["nr"] > 128)
    assert any(r["ndr"] > 0 for r in el if r["dir"] == 0)
    cap = 64
    small = _layouts("w64", cap_entries=cap)
    room = 10 * (cap + 8)
    need = {(r["block"], r["dir"]): 8 * r["slots"] + r["ndr"] * r["nrp"] for r in el}
    assert any(v > room for v in need.values())
    for r in small:
        k = (r["block"], r["dir"])
        assert r["eligible"] == (k in need and need[k] <= room)
