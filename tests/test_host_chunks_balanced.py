"""The even split of the fused build's work list and its dispatch order by records (hyperslam_amd/csrc/host_structure.hpp:
build_chunks_balanced, order_chunks_by_records) against an independent numpy restatement of their rules, on CPU.

Rules restated here:
  1. per landmark group, k = the chunks the greedy fill under (L landmarks, R records) makes; cut j = 1 .. k - 1 goes behind the landmark
     whose cumulative record count is nearest to j total / k (ties: the smaller index; every chunk keeps a landmark). When such a chunk
     has more than L landmarks or more records than the largest greedy chunk of the group: greedy fill under L and the smallest record
     limit that needs at most k chunks, every chunk leaving one landmark for each chunk behind it.
  2. dispatch: weight = records, then landmarks, then the smaller chunk id; n_cu < n <= 2 n_cu: the heaviest chunks on the lone compute
     units, the rest heaviest (first slot) with lightest (second slot); otherwise heaviest first."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from test_host_structure import expected, expected_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(138, 14), (84, 8), (112, 11), (40, 3)]
# (seed, k, n_cp, n_lm, n_px): the generators of test_host_structure.py::test_chunks_and_dispatch_order
GENERATORS = [(11, 4, 16, 40, 700), (12, 4, 63, 479, 9000), (13, 6, 24, 60, 800), (14, 5, 40, 300, 3000), (15, 4, 10, 12, 90), (16, 4, 128, 2000, 20000),
              (17, 4, 128, 5000, 50000)]


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("chunks") / "chunks_balanced_dump")
    subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "hyperslam_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "helpers", "chunks_balanced_dump.cpp")], stderr=subprocess.DEVNULL)
    return exe


def run(exe, tmp_path, k, n_cp, n_lm, t0, dt, stamp, lm, R, L):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    with open(src, "wb") as f:
        f.write(struct.pack("=5i2d", k, n_cp, n_lm, len(stamp), 0, t0, dt))
        f.write(np.asarray(stamp, dtype="<f8").tobytes())
        f.write(np.asarray(lm, dtype="<i4").tobytes())
    subprocess.check_call([exe, src, dst, str(R), str(L)])
    out = {}
    for line in open(dst):
        parts = line.split()
        assert parts[0] != "error", line
        out[parts[0]] = np.array(parts[2:], dtype=np.int64)
        assert len(out[parts[0]]) == int(parts[1])
    return out


# ---- numpy restatement ----

def greedy_bounds(per, L, C):
    """Boundaries of the greedy fill of one group under (L, C)."""
    b, d = [0], 0
    while d < len(per):
        e, cnt = d, 0
        while e < len(per) and e - d < L and cnt + per[e] <= C:
            cnt += per[e]
            e += 1
        assert e > d
        b.append(e)
        d = e
    return b


def largest(per, b):
    return max(int(per[lo:hi].sum()) for lo, hi in zip(b[:-1], b[1:]))


def even_bounds(per, k, cap, L, stats=None):
    n, cum = len(per), np.concatenate([[0], np.cumsum(per)])
    b = [0]
    for j in range(1, k):
        cand = np.arange(b[-1] + 1, n - (k - j) + 1)
        b.append(int(cand[np.argmin(np.abs(cum[cand] * k - j * cum[-1]))]))  # (argmin: the first of equal minima)
    b.append(n)
    if max(np.diff(b)) <= L and largest(per, b) <= cap:
        return b
    if stats is not None:
        stats["fallback"] = stats.get("fallback", 0) + 1
    C = next(c for c in range(int(per.max()), cap + 1) if len(greedy_bounds(per, L, c)) - 1 <= k)
    b, d = [0], 0
    for j in range(k):
        e, cnt = d, 0
        while e < n - (k - 1 - j) and e - d < L and cnt + per[e] <= C:
            cnt += per[e]
            e += 1
        b.append(e)
        d = e
    assert d == n
    return b


def balanced_chunks(want, n_cp, R, L, stats=None):
    """(ch_ptr, gw_ptr, gw_cf, desc) of build_chunks_balanced, or None where it declines."""
    lm_ptr, cf_ptr, cfirst = want["lm_ptr"], want["cf_ptr"], want["lm_cfirst"]
    per_lm = np.diff(lm_ptr)
    n_obs = int(np.count_nonzero(per_lm))
    if n_obs and per_lm[:n_obs].max() > R:
        return None
    ch_ptr, gw_ptr, gw_cf = [], [0] * (n_cp + 1), []
    for c in range(n_cp):
        gw_ptr[c] = len(gw_cf)
        d0, d1 = min(cf_ptr[c], n_obs), min(cf_ptr[c + 1], n_obs)
        if d1 > d0:
            per = per_lm[d0:d1]
            g = greedy_bounds(per, L, R)
            b = even_bounds(per, len(g) - 1, largest(per, g), L, stats)
            ch_ptr += [d0 + x for x in b[:-1]]
            gw_cf += [c] * (len(b) - 1)
    gw_ptr[n_cp] = len(gw_cf)
    ch_ptr.append(n_obs), gw_cf.append(0)
    desc = [[lo, hi - lo, cfirst[lo], lm_ptr[lo], lm_ptr[hi] - lm_ptr[lo], w, 0, 0] for w, (lo, hi) in enumerate(zip(ch_ptr[:-1], ch_ptr[1:]))]
    return np.array(ch_ptr), np.array(gw_ptr), np.array(gw_cf), np.array(desc, dtype=np.int64).reshape(-1, 8)


def dispatch_by_records(desc, n_cu):
    n = len(desc)
    if n <= 1:
        return desc
    order = np.lexsort((desc[:, 5], -desc[:, 1], -desc[:, 4]))  # records, then landmarks (both descending), then chunk id
    slot = np.empty(n, dtype=np.int64)
    if n_cu < n <= 2 * n_cu:
        n_lone, n_pair = 2 * n_cu - n, n - n_cu
        slot[n_pair:n_pair + n_lone] = order[:n_lone]
        slot[:n_pair] = order[n_lone:n_lone + n_pair]
        slot[n_cu:] = order[::-1][:n_pair]
    else:
        slot[:] = order
    return desc[slot]


def heaviest_cu(desc, n_cu):
    """Most records on one compute unit (workgroup w runs on unit w mod n_cu)."""
    return int(np.bincount(np.arange(len(desc)) % n_cu, weights=desc[:, 4]).max()) if len(desc) else 0


def check(got, want, k, n_cp, R, L, stats=None):
    """Everything the dumper wrote against the restatement and the properties of the split."""
    per_lm = np.diff(want["lm_ptr"])
    for name in ("lm_ptr", "cf_ptr", "lm_cfirst"):
        assert np.array_equal(got[name], want[name]), name
    if "declined" in got:
        assert balanced_chunks(want, n_cp, R, L) is None
        return None
    _, gw_ptr_greedy, _, desc_greedy = expected_chunks(want, k, n_cp, R, L)
    if len(desc_greedy):
        assert np.array_equal(got["greedy_ch_desc"].reshape(-1, 8), desc_greedy)
    out = {}
    ch_ptr, gw_ptr, gw_cf, desc = balanced_chunks(want, n_cp, R, L, stats)
    assert np.array_equal(got["ch_ptr"], ch_ptr)
    assert np.array_equal(got["gw_ptr"], gw_ptr) and np.array_equal(got["gw_cf"], gw_cf)
    n = len(ch_ptr) - 1
    d = got["ch_desc"].reshape(-1, 8)[:n]
    assert np.array_equal(d, desc)
    # properties: consecutive landmarks, every record in exactly one chunk, the limits, one first control point per chunk
    assert d[:, 4].sum() == per_lm.sum()
    if n:
        assert np.array_equal(d[:, 0] + d[:, 1], np.append(d[1:, 0], ch_ptr[-1])) and d[0, 0] == 0
        assert np.array_equal(d[:, 3] + d[:, 4], np.append(d[1:, 3], per_lm.sum())) and d[0, 3] == 0
        assert d[:, 1].min() >= 1 and d[:, 1].max() <= L and d[:, 4].max() <= R
    for w in range(n):
        assert (want["lm_cfirst"][d[w, 0]:d[w, 0] + d[w, 1]] == gw_cf[w]).all() and d[w, 2] == gw_cf[w]
    # per group: greedy's chunk count, no chunk larger than greedy's largest
    assert np.array_equal(gw_ptr, gw_ptr_greedy)
    for c in range(n_cp):
        if gw_ptr[c + 1] > gw_ptr[c]:
            assert d[gw_ptr[c]:gw_ptr[c + 1], 4].max() <= desc_greedy[gw_ptr_greedy[c]:gw_ptr_greedy[c + 1], 4].max(), c
    for n_cu in (8, 256):
        o = got["ch_desc_cu%d" % n_cu].reshape(-1, 8)[:n]
        assert sorted(o[:, 5]) == list(range(n))  # a permutation: every chunk dispatched once ...
        assert np.array_equal(o[np.argsort(o[:, 5])], desc)  # ... with its descriptor and its partial slot unchanged
        assert np.array_equal(o, dispatch_by_records(desc, n_cu)), n_cu
        out["even", n_cu] = o
    out["greedy", 256] = got["greedy_ch_desc_cu256"].reshape(-1, 8)[:len(desc_greedy)] if len(desc_greedy) else desc_greedy
    return out


@pytest.mark.parametrize("R,L", GEOMETRIES)
@pytest.mark.parametrize("seed,k,n_cp,n_lm,n_px", GENERATORS)
def test_balanced_chunks_and_dispatch_by_records(seed, k, n_cp, n_lm, n_px, R, L, dumper, tmp_path):
    rng = np.random.default_rng(seed)
    t0, dt = 0.0, 0.05
    lo, hi = t0 + (k - 1) // 2 * dt, t0 + ((k - 1) // 2 + n_cp - k + 1) * dt
    lm = rng.integers(0, n_lm, n_px)
    anchor = rng.uniform(lo, hi, n_lm)
    stamp = np.clip(anchor[lm] + rng.uniform(-3 * dt, 3 * dt, n_px), lo + 1e-9, hi - 1e-9)
    none = np.array([], dtype=np.float64)
    got = run(dumper, tmp_path, k, n_cp, n_lm, t0, dt, stamp, lm, R, L)
    want = expected(k, n_cp, n_lm, t0, dt, stamp, lm, none, none.astype(np.int64))
    check(got, want, k, n_cp, R, L)


def crafted(groups, n_cp, extra_landmarks=0):
    """Order-4 window on the knots 0, 1, 2, ...: groups = {first control point: [records of each of its landmarks]}; landmark ids in table order."""
    stamp, lm, n_lm = [], [], 0
    for c in sorted(groups):
        for r in groups[c]:
            stamp += [c + 1.5] * r  # order 4: first control point = floor(stamp) - 1
            lm += [n_lm] * r
            n_lm += 1
    return dict(k=4, n_cp=n_cp, n_lm=n_lm + extra_landmarks, t0=0.0, dt=1.0, stamp=np.array(stamp, dtype=np.float64), lm=np.array(lm, dtype=np.int64))


def run_crafted(dumper, tmp_path, win, R, L, stats=None):
    none = np.array([], dtype=np.float64)
    got = run(dumper, tmp_path, win["k"], win["n_cp"], win["n_lm"], win["t0"], win["dt"], win["stamp"], win["lm"], R, L)
    want = expected(win["k"], win["n_cp"], win["n_lm"], win["t0"], win["dt"], win["stamp"], win["lm"].astype(np.int64), none, none.astype(np.int64))
    return got, check(got, want, win["k"], win["n_cp"], R, L, stats)


def test_edge_cases(dumper, tmp_path):
    R, L = 40, 3
    # a group of one landmark; a landmark of exactly R records between two others (a chunk of one); unobserved landmarks last
    got, _ = run_crafted(dumper, tmp_path, crafted({2: [5], 4: [3, R, 2], 7: [1, 1, 1, 1]}, 12, extra_landmarks=3), R, L)
    d = got["ch_desc"].reshape(-1, 8)
    assert d[:, 1].tolist() == [1, 1, 1, 1, 2, 2] and d[:, 4].tolist() == [5, 3, R, 2, 2, 2]
    assert got["ch_ptr"][-1] == 8  # the three unobserved landmarks are in no chunk
    # R + 1 records on one landmark: declined
    got, _ = run_crafted(dumper, tmp_path, crafted({2: [5], 4: [3, R + 1, 2]}, 12), R, L)
    assert "declined" in got
    # no landmarks at all
    got, _ = run_crafted(dumper, tmp_path, crafted({}, 8), R, L)
    assert got["ch_ptr"].tolist() == [0] and got["gw_ptr"].tolist() == [0] * 9
    # proportional cuts that break L (30 | 1 | 1 1 1 1 1): the group falls back to the greedy fill under the smallest record limit
    stats = {}
    got, _ = run_crafted(dumper, tmp_path, crafted({3: [30, 1, 1, 1, 1, 1, 1]}, 8), R, L, stats)
    assert stats.get("fallback", 0) >= 1
    assert got["ch_desc"].reshape(-1, 8)[:, 1].tolist() == [1, 3, 3]
    # an even group splits evenly where the greedy fill leaves a remainder: 40 landmarks of 10 records, L = 12
    got, _ = run_crafted(dumper, tmp_path, crafted({0: [10] * 40}, 8), 128, 12)
    assert got["greedy_ch_desc"].reshape(-1, 8)[:, 1].tolist() == [12, 12, 12, 4] and got["ch_desc"].reshape(-1, 8)[:, 1].tolist() == [10, 10, 10, 10]


@pytest.mark.parametrize("seed", [31, 32, 33, 34])
def test_uneven_landmarks(seed, dumper, tmp_path):
    """Landmarks of very different record counts: the fallback."""
    rng = np.random.default_rng(seed)
    R, L = [(40, 3), (84, 8)][seed % 2]
    groups = {c: np.minimum(R, np.where(rng.random(n) < 0.25, rng.integers(R // 3, R + 1, n), rng.integers(1, 4, n))).tolist()
              for c, n in enumerate(rng.integers(1, 30, 20))}
    stats = {}
    run_crafted(dumper, tmp_path, crafted(groups, 24), R, L, stats)
    assert stats.get("fallback", 0) >= 1  # (the generator is meant to reach it)


def test_bench_window(dumper, tmp_path):
    """The window bench.py measures (128 control points, 5 000 landmarks of 10 records) on 256 compute units: 475 chunks either way, 240
    records on the heaviest unit with the greedy fill and its pairing, 210 with the even split paired by records."""
    from hyperslam_amd import synthetic
    w = synthetic.config1()
    k, n_cp, n_lm = int(w.order), int(w.control_points.shape[0]), len(w.landmarks)
    none = np.array([], dtype=np.float64)
    got = run(dumper, tmp_path, k, n_cp, n_lm, w.t0, w.dt, w.pixel_stamps, w.pixel_landmark, 128, 12)
    want = expected(k, n_cp, n_lm, w.t0, w.dt, w.pixel_stamps, w.pixel_landmark.astype(np.int64), none, none.astype(np.int64))
    out = check(got, want, k, n_cp, 128, 12)
    assert len(out["greedy", 256]) == 475 and heaviest_cu(out["greedy", 256], 256) == 240
    assert len(out["even", 256]) == 475 and heaviest_cu(out["even", 256], 256) == 210
    assert out["greedy", 256][:, 1].max() == 12 and out["even", 256][:, 1].max() == 12
