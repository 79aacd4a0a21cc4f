"""Caller-made oriented-keypoint records for the SIFT selection stage (``vo_sift_testing_select``,
``oracle/sift_ref.select_keypoints``): the case generators that tests/test_sift_select_ref.py
(CPU) and tests/test_gpu_sift_select.py share.  A plain helper module, not a conftest.

Every generator returns ``(okp, counts, nfeatures, cap_img)``: okp (batch, cap_img, 8) float32
records ``x, y, size, angle, response, octave-word bits, 0, 0`` in doubled-image units at
shuffled slots, counts (batch,) int32.  x and y are float32 values in [4.5, 32768) (the range
``sift_keys_kernel``'s 27-bit keys assume), some adjacent in float32, with equal-x runs that
differ only in y; sizes and angles come from small pools so that duplicates occur; responses are
strictly positive normal float32 values; octave words are positive (octave | layer << 8 |
offset byte << 16, as the detector writes them).

An image is described as a list of runs in sorted (x, y) order, so a generator decides where in
the sorted order a run sits; a run is a list of (size, angle, response, word) records that share
one (x, y) plus the order its records arrive in after the (stable) key sort: by slot number.

``CLAIMS[name]`` states the shape each case is built to have; ``facts(case)`` measures it from
the raw arrays (without the reference), and the CPU tests compare the two, so that a later edit
of a generator cannot quietly empty a GPU test.
"""

from __future__ import annotations

import functools

import numpy as np

F = np.float32
K_RUN_MAX = 8        # csrc/sift_desc.hip kRunMax: longer runs take the insertion sort
K_LONG_QUEUE = 2048  # csrc/sift_desc.hip kLongQueue: more runs of >= 3 records are found again by a rescan
XY_LO, XY_HI = F(4.5), F(32768.0)

SIZES = np.array([3.2, 4.031747, 5.0796833, 6.4, 8.063494], F)
ANGLES = np.array([0.0, 12.5, 180.25, 359.875], F)


def word(o: int, layer: int, xi: int) -> int:
    """An octave word as the detector writes it (before the first-octave shift): positive."""
    return (o & 7) | ((1 + layer % 3) << 8) | ((xi & 255) << 16)


class Run:
    """Records (size, angle, response, word) that share one (x, y); arrival: 'shuffle', or
    'reverse' / 'forward' for the comparator order reversed / kept in slot order."""

    def __init__(self, recs, arrival="shuffle"):
        self.recs = [(F(s), F(a), F(r), int(w)) for s, a, r, w in recs]
        self.arrival = arrival


def _cmp_key(r):
    return (-r[0], r[1], -r[2], -r[3])


def _values(rng, n):
    """n float32 coordinate values in [4.5, 32768): both ends, random ones, float32 neighbours."""
    v = [XY_LO, np.nextafter(XY_LO, XY_HI), np.nextafter(XY_HI, XY_LO), np.nextafter(np.nextafter(XY_HI, XY_LO), XY_LO)]
    while len(v) < n:
        x = F(rng.uniform(4.5, 32767.0)) if rng.random() < 0.5 else F(rng.uniform(4.5, 64.0))
        v += [x, np.nextafter(x, XY_HI)]
    return np.unique(np.array(v[:n], F))


def coord_pool(rng, n):
    """n distinct (x, y) pairs sorted as the keys sort (x, then y); about 1.5 sqrt(n) distinct x
    values, so most x values head several runs that differ only in y."""
    k = max(3, int(1.5 * np.sqrt(n)) + 2)
    xs, ys = _values(rng, k), _values(rng, k + 3)
    pairs = set()
    while len(pairs) < n:
        pairs.add((float(xs[rng.integers(len(xs))]), float(ys[rng.integers(len(ys))])))
    return sorted(pairs)


def rand_run(rng, length, arrival="shuffle"):
    """A run with sizes / angles from the pools (so duplicates occur) and random responses."""
    recs = []
    for _ in range(length):
        r = F(rng.uniform(0.01, 0.2))
        recs.append((SIZES[rng.integers(3)], ANGLES[rng.integers(3)], r, word(rng.integers(8), rng.integers(3),
                                                                                  rng.integers(256))))
    return Run(recs, arrival)


def single(resp, i=0):
    return Run([(SIZES[i % 5], ANGLES[i % 4], resp, word(i, i, i * 7))])


def assemble(images, cap_img, nfeatures, rng, pool=None, counts=None):
    """images: per image the list of runs in sorted order -> (okp, counts, nfeatures, cap_img).
    pool: shared sorted (x, y) pairs the images draw their runs' positions from (else a pool of
    its own per image)."""
    batch = len(images)
    okp = np.zeros((batch, cap_img, 8), F)
    cnt = np.zeros(batch, np.int32)
    for b, runs in enumerate(images):
        n = sum(len(r.recs) for r in runs)
        assert n <= cap_img
        cnt[b] = n
        if pool is None:
            xy = coord_pool(rng, len(runs))
        else:
            xy = [pool[i] for i in sorted(rng.choice(len(pool), len(runs), replace=False))]
        slots = rng.permutation(n)
        at = 0
        for (x, y), run in zip(xy, runs):
            L = len(run.recs)
            s = slots[at:at + L]
            at += L
            recs = run.recs
            if run.arrival != "shuffle":
                recs = sorted(recs, key=_cmp_key)
                s = np.sort(s)[::-1] if run.arrival == "reverse" else np.sort(s)
            for slot, (sz, an, rs, wd) in zip(s, recs):
                okp[b, slot, :5] = (x, y, sz, an, rs)
                okp[b, slot, 5:6].view(np.int32)[0] = wd
    if counts is not None:
        cnt = np.asarray(counts, np.int32)
    return okp, cnt, int(nfeatures), int(cap_img)


# ---- the cases ------------------------------------------------------------------------------

def _fill(rng, n_runs, max_len=3):
    return [rand_run(rng, int(rng.integers(1, max_len + 1))) for _ in range(n_runs)]


def run_lengths():
    """Lengths 1..12 and 40, each twice, in one image (pair, register and insertion paths)."""
    rng = np.random.default_rng(101)
    runs = [rand_run(rng, L) for L in list(range(1, 13)) + [40] for _ in range(2)]
    runs += [rand_run(rng, 1) for _ in range(30)] + [rand_run(rng, 2) for _ in range(10)]
    runs = [runs[i] for i in rng.permutation(len(runs))]
    return assemble([runs], 320, 0, rng)


RUN_TAILS = [(1, 0), (2, 0), (3, 0), (7, 0), (7, 1), (7, 2), (8, 0), (8, 1), (8, 2), (9, 0), (9, 1), (9, 2)]


def run_tails():
    """One image per (L, t): a run of L records followed by t single records ends the image's
    records (run head at each of the last three positions; 7, 8, 9 against the end)."""
    rng = np.random.default_rng(102)
    images = [_fill(rng, 20) + [rand_run(rng, L)] + [rand_run(rng, 1) for _ in range(t)] for L, t in RUN_TAILS]
    return assemble(images, 128, 0, rng)


LEVELS = ("size", "angle", "response", "octave")


def level_run(level, length, arrival):
    """A run whose order is decided at comparator level `level`: the earlier fields are shared,
    the level's field takes length / 2 values (equal pairs), every other equal pair is decided by
    the next level and the rest are identical records."""
    k = LEVELS.index(level)
    recs = []
    for i in range(length):
        f = [0, 0, 0, 0]
        f[k] = 1 + i // 2
        if k + 1 < 4 and (i // 2) % 2 == 0:
            f[k + 1] = i % 2
        recs.append((F(3.0 + 0.25 * f[0]), F(7.5 * f[1]), F(0.01 * (f[2] + 1)), word(f[3], f[3] // 8, 5 + f[3] // 24)))
    return Run(recs, arrival)


def _levels(lengths, seed):
    rng = np.random.default_rng(seed)
    runs = [level_run(lv, L, arr) for lv in LEVELS for L in lengths for arr in ("reverse", "forward", "shuffle")]
    runs += _fill(rng, 20, 2)
    runs = [runs[i] for i in rng.permutation(len(runs))]
    return assemble([runs], 1024, 0, rng)


def levels_register():
    """Runs of 3, 4, 5, 8 records (sorted in registers) decided by each comparator level."""
    return _levels((3, 4, 5, 8), 103)


def levels_insertion():
    """Runs of 9 and 40 records (insertion sort) decided by each comparator level."""
    return _levels((9, 40), 104)


def _dups(groups, n_runs, seed, extra=()):
    """n_runs runs, each made of groups (m duplicates after one record each): the record has the
    run's top response and its duplicates (same size and angle) responses just below, all far above
    the 100 single records.  nfeatures cuts among the singles: the dropped duplicates must not
    count towards the rank."""
    rng = np.random.default_rng(seed)
    runs = []
    for j in range(n_runs):
        recs = []
        for g, m in enumerate(groups):
            top = 0.9 - 0.001 * j - 0.0001 * g
            recs.append((SIZES[g], ANGLES[g], top, word(j, g, j)))
            recs += [(SIZES[g], ANGLES[g], top - 0.00001 * (d + 1), word(j + d, g, d)) for d in range(m)]
        runs.append(Run(recs))
    runs += list(extra)
    kept = sum(len(groups) for _ in range(n_runs)) + len(extra)
    runs += [single(0.1 + 0.003 * i, i) for i in range(100)]
    runs = [runs[i] for i in rng.permutation(len(runs))]
    return assemble([runs], 512, kept + 20, rng)


def dups_pair():
    """30 pairs that are one record and its duplicate (the pair path of the first pass)."""
    return _dups((1,), 30, 105)


def dups_register():
    """10 runs of 7: a record with 3 duplicates and one with 2 (the register path)."""
    return _dups((3, 2), 10, 106)


def dups_insertion():
    """8 runs of 11 (a record with 6 duplicates, one with 3) and a run of 40 that is one record
    and 39 duplicates (the insertion path)."""
    one = Run([(SIZES[4], ANGLES[3], 0.95 - 0.0001 * d, word(d, d, d)) for d in range(40)])
    return _dups((6, 3), 8, 107, extra=[one])


def _long_queue(n_long):
    rng = np.random.default_rng(108)
    lengths = [L for L in range(4, 11) for _ in range(30)] + [3] * (n_long - 210)
    runs = [rand_run(rng, L) for L in lengths]
    runs += [rand_run(rng, 1) for _ in range(300)] + [rand_run(rng, 2) for _ in range(200)]
    runs = [runs[i] for i in rng.permutation(len(runs))]
    return assemble([runs], 8192, 3000, rng)


def long_queue_2100():
    """2100 runs of 3..10 records in one image: the queue of long runs overflows (rescan)."""
    return _long_queue(2100)


def long_queue_2049():
    """2049 runs of 3..10 records: one more than the queue holds."""
    return _long_queue(2049)


def long_queue_2048():
    """2048 runs of 3..10 records: the queue is exactly full (no rescan)."""
    return _long_queue(2048)


NF_KEPT = 110


def _nf_image(nfeatures):
    """40 singles, 20 pairs, 10 pairs that are duplicates, 10 triples with one duplicate: 110 kept,
    all responses distinct."""
    rng = np.random.default_rng(109)
    resp = iter(F(0.02) + F(0.0007) * np.arange(400, dtype=F)[rng.permutation(400)])
    rec = lambda s, a: (SIZES[s], ANGLES[a], next(resp), word(s, a, s + a))
    runs = [Run([rec(i % 5, i % 4)]) for i in range(40)]
    runs += [Run([rec(0, 1), rec(1, 1)]) for _ in range(20)]
    runs += [Run([rec(2, 2), rec(2, 2)]) for _ in range(10)]
    runs += [Run([rec(3, 0), rec(3, 3), rec(3, 0)]) for _ in range(10)]
    runs = [runs[i] for i in rng.permutation(len(runs))]
    return assemble([runs], 160, nfeatures, rng)


def nf_1():
    return _nf_image(1)


def nf_kept_minus_1():
    return _nf_image(NF_KEPT - 1)


def nf_kept():
    return _nf_image(NF_KEPT)


def nf_kept_plus_1():
    return _nf_image(NF_KEPT + 1)


def all_equal():
    """Every response equal: 100 singles and 10 pairs, nfeatures 10, all 120 stay."""
    rng = np.random.default_rng(110)
    runs = [single(0.05, i) for i in range(100)] + [Run([(SIZES[0], ANGLES[0], 0.05, word(1, 1, 1)),
                                                         (SIZES[1], ANGLES[0], 0.05, word(1, 1, 1))]) for _ in range(10)]
    return assemble([runs], 128, 10, rng)


def tie_50():
    """30 responses above, 50 tied, 100 below; the rank (55) falls inside the tie: 80 stay."""
    rng = np.random.default_rng(111)
    runs = [single(0.2 + 0.001 * i, i) for i in range(30)] + [single(0.1, i) for i in range(50)]
    runs += [single(0.01 + 0.0005 * i, i) for i in range(100)]
    runs = [runs[i] for i in rng.permutation(len(runs))]
    return assemble([runs], 192, 55, rng)


def _bits(u):
    return np.array([u], np.uint32).view(F)[0]


RADIX_NF = 100


def only_byte():
    """Image k (0..3): 200 single records whose response bits differ only in byte k."""
    rng = np.random.default_rng(112)
    images = []
    for k in range(4):
        base = 0x3D804020 & ~(255 << (8 * k)) if k < 3 else 0x00804020
        vals = rng.integers(1, 0x7F, 200) if k == 3 else rng.integers(0, 256, 200)
        images.append([single(_bits(base | (int(v) << (8 * k))), i) for i, v in enumerate(vals)])
    return assemble(images, 256, RADIX_NF, rng)


# (pass, digit): the byte of the response bits and the value the radix select must pick there
DIGITS = [(p, d) for p in (0, 1, 2) for d in (255, 252, 3, 0)] + [(3, 3), (3, 0), (0, 131), (0, 128), (0, 127), (0, 124)]


def digits():
    """One image per (pass, digit) of DIGITS: 60 responses whose byte `pass` is above the digit
    (none for 255), 80 at the digit, 60 below (none for 0), the bytes under it random from a small
    pool and the bytes over it shared: rank 100 falls among the 80, so the pass picks the digit
    (255: lane 0's first, 252: lane 0's last, 3: lane 63's first, 0: lane 63's last)."""
    rng = np.random.default_rng(113)
    low_pool = np.array([0, 3, 64, 252, 255])
    images = []
    for p, d in DIGITS:
        top = 0x7E if p == 3 else 255
        n_above, n_below = (60 if d < top else 0), (60 if d > 0 else 0)
        n_tie = 200 - n_above - n_below
        vals = [int(rng.integers(d + 1, top + 1)) for _ in range(n_above)] + [d] * n_tie
        vals += [int(rng.integers(0, d)) for _ in range(n_below)]
        runs = []
        for i, v in enumerate(vals):
            u = 0x3D800000 if p < 2 else (0x3D000000 if p == 2 else 0x00800000)
            u = (u & ~(255 << (8 * p))) | (v << (8 * p))
            for q in range(p):
                keep_normal = 0x80 if (p == 3 and q == 2) else 0
                u = (u & ~(255 << (8 * q))) | ((int(low_pool[rng.integers(5)]) | keep_normal) << (8 * q))
            runs.append(single(_bits(u), i))
        images.append([runs[i] for i in rng.permutation(len(runs))])
    return assemble(images, 256, RADIX_NF, rng)


POSITION_N = [0, 1, 2, 3, 1023, 1024, 1025, 4095, 4096, 4097, 4200, 4200, 4200]
# per image: {start position in the sorted order: run length} of the runs placed on purpose
POSITION_RUNS = [{}, {0: 1}, {0: 2}, {0: 3}, {1020: 3}, {1022: 2}, {1023: 2}, {1022: 3, 4092: 3}, {1023: 3, 4094: 2},
                 {1023: 2, 4095: 2}, {1022: 3, 4094: 3}, {1023: 3, 4095: 3}, {1021: 5, 4092: 9}]


def positions():
    """n on both sides of 1024 and 4096 (four records per thread and round of 4096), with runs of
    2 and 3 records (and of 5 and 9) across the 1023|1024 and 4095|4096 positions."""
    rng = np.random.default_rng(114)
    images = []
    for n, placed in zip(POSITION_N, POSITION_RUNS):
        runs, at = [], 0
        while at < n:
            if at in placed:
                L = placed[at]
            else:
                gap = min([s for s in placed if s > at] + [n]) - at
                L = min(gap, int(rng.integers(1, 4)) if rng.random() < 0.2 else 1)
            runs.append(rand_run(rng, L))
            at += L
        images.append(runs)
    return assemble(images, 4200, 1000, rng)


BATCH_COUNTS = {1: [37], 2: [0, 40], 3: [25, 0, 31], 4: [10, 33, 17, 0], 5: [0, 29, 0, 41, 12]}


def _batch(batch, seed):
    rng = np.random.default_rng(seed)
    cap = 16 if batch == 256 else 48
    if batch == 256:
        counts = rng.integers(0, cap + 1, batch)
        counts[[0, 100, 255]] = 0
        counts[[1, 254]] = cap
    else:
        counts = BATCH_COUNTS[batch]
    images = []
    for n in counts:
        runs, at = [], 0
        while at < n:
            L = min(int(n) - at, int(rng.integers(1, 5)))
            runs.append(rand_run(rng, L))
            at += L
        images.append(runs)
    # shared, and hardly larger than the largest image needs: the same (x, y) values recur in every image
    pool = coord_pool(rng, max(len(runs) for runs in images) + 2)
    return assemble(images, cap, 8 if batch == 256 else 12, rng, pool=pool)


def batch_1():
    return _batch(1, 121)


def batch_2():
    return _batch(2, 122)


def batch_3():
    return _batch(3, 123)


def batch_4():
    return _batch(4, 124)


def batch_5():
    return _batch(5, 125)


def batch_256():
    return _batch(256, 126)


OVERFLOW_COUNTS = [10, 20, 5]


def overflow():
    """The middle image reports 20 records at a capacity of 16."""
    rng = np.random.default_rng(127)
    images = [[rand_run(rng, 1) for _ in range(n)] for n in (10, 16, 5)]
    return assemble(images, 16, 0, rng, counts=OVERFLOW_COUNTS)


GENERATORS = [run_lengths, run_tails, levels_register, levels_insertion, dups_pair, dups_register, dups_insertion,
              long_queue_2100, long_queue_2049, long_queue_2048, nf_1, nf_kept_minus_1, nf_kept, nf_kept_plus_1,
              all_equal, tie_50, only_byte, digits, positions, batch_1, batch_2, batch_3, batch_4, batch_5, batch_256]
NAMES = [g.__name__ for g in GENERATORS]


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case, built once (read-only arrays)."""
    okp, counts, nfeatures, cap_img = globals()[name]()
    okp.setflags(write=False)
    counts.setflags(write=False)
    return okp, counts, nfeatures, cap_img


def records(okp_img, n):
    """The keypoint dicts ``oracle/sift_ref.select_keypoints`` takes, of an image's first n slots."""
    w = okp_img[:, 5].view(np.int32)
    return [dict(x=okp_img[i, 0], y=okp_img[i, 1], size=okp_img[i, 2], angle=okp_img[i, 3], response=okp_img[i, 4],
                 octave=int(w[i])) for i in range(n)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per image of the named case: the slots ``select_keypoints`` keeps, in output order."""
    from oracle import sift_ref

    okp, counts, nfeatures, cap_img = case(name)
    return tuple(np.array(sift_ref.select_keypoints(records(okp[b], min(int(counts[b]), cap_img)), nfeatures)[1],
                          np.int64) for b in range(len(counts)))


# ---- the shape of a case, measured from its arrays -------------------------------------------

def image_facts(okp_img, n, nfeatures):
    """The runs of an image's n records in sorted order and what retainBest meets: a dict of
    starts / lengths (arrays, in sorted order), nlong (runs of >= 3), longest, dups (records
    removeDuplicatedSorted drops: a run's records less its distinct (size, angle) pairs), kept,
    and, when the cut binds, thr_bits (the nfeatures-th largest kept response), tie (kept records at
    it), sep_byte (the highest byte in which it differs from the nearest other kept responses)."""
    r = okp_img[:n]
    out = dict(n=n, starts=np.zeros(0, np.int64), lengths=np.zeros(0, np.int64), nlong=0, longest=0, dups=0, kept=0,
               thr_bits=None, tie=0, sep_byte=None)
    if n == 0:
        return out
    order = np.lexsort((r[:, 1], r[:, 0]))
    s = r[order]
    head = np.ones(n, bool)
    head[1:] = (s[1:, 0] != s[:-1, 0]) | (s[1:, 1] != s[:-1, 1])
    starts = np.flatnonzero(head)
    lengths = np.diff(np.append(starts, n))
    best = {}  # (x, y, size, angle) -> the largest response: the record that stays
    for x, y, sz, an, rs in s[:, :5]:
        k = (x, y, sz, an)
        best[k] = max(best.get(k, rs), rs)
    kept = np.sort(np.array(list(best.values()), F).view(np.uint32))[::-1]  # positive floats order as their bits
    out.update(starts=starts, lengths=lengths, nlong=int((lengths >= 3).sum()), longest=int(lengths.max()),
               dups=n - len(best), kept=len(kept))
    if nfeatures > 0 and len(kept) > nfeatures:
        t = int(kept[nfeatures - 1])
        others = [int(v) for v in (kept[kept > t][-1:].tolist() + kept[kept < t][:1].tolist())]
        out.update(thr_bits=t, tie=int((kept == t).sum()),
                   sep_byte=max(((v ^ t).bit_length() - 1) // 8 for v in others) if others else None)
    return out


def facts(name):
    okp, counts, nfeatures, cap_img = case(name)
    return [image_facts(okp[b], min(int(counts[b]), cap_img), nfeatures) for b in range(len(counts))]


# What each case is built to be.  Per case, lists hold one entry per image; a scalar holds for the
# single image.  nlong: runs of >= 3 records; lengths: the exact set of run lengths present;
# dups: records removeDuplicatedSorted drops; tie: kept records at the retainBest threshold (0: the
# cut does not bind); sep_byte: the byte of the response bits that separates the threshold from its
# neighbours; digit: (pass, digit) the radix select picks; placed / last_runs: runs at given
# positions of the sorted order; shared_xy: (x, y) values that occur in more than one image.
_MIXED = dict(lengths=set(range(1, 13)) | {40}, longest=40, nlong=22)
CLAIMS = {
    "run_lengths": dict(_MIXED, tie=0),
    "run_tails": dict(last_runs=RUN_TAILS, tie=0),
    "levels_register": dict(lengths={1, 2, 3, 4, 5, 8}, longest=8, nlong=48, tie=0),
    "levels_insertion": dict(lengths={1, 2, 9, 40}, longest=40, nlong=24, tie=0),
    "dups_pair": dict(lengths={1, 2}, longest=2, nlong=0, dups=30, kept=130, tie=1),
    "dups_register": dict(lengths={1, 7}, longest=7, nlong=10, dups=50, kept=120, tie=1),
    "dups_insertion": dict(lengths={1, 11, 40}, longest=40, nlong=9, dups=8 * 9 + 39, kept=117, tie=1),
    "long_queue_2100": dict(lengths=set(range(1, 11)), longest=10, nlong=2100),
    "long_queue_2049": dict(lengths=set(range(1, 11)), longest=10, nlong=2049),
    "long_queue_2048": dict(lengths=set(range(1, 11)), longest=10, nlong=2048),
    "nf_1": dict(lengths={1, 2, 3}, longest=3, nlong=10, dups=20, kept=NF_KEPT, tie=1),
    "nf_kept_minus_1": dict(lengths={1, 2, 3}, longest=3, nlong=10, dups=20, kept=NF_KEPT, tie=1),
    "nf_kept": dict(lengths={1, 2, 3}, longest=3, nlong=10, dups=20, kept=NF_KEPT, tie=0),
    "nf_kept_plus_1": dict(lengths={1, 2, 3}, longest=3, nlong=10, dups=20, kept=NF_KEPT, tie=0),
    "all_equal": dict(lengths={1, 2}, longest=2, nlong=0, dups=0, kept=120, tie=120),
    "tie_50": dict(lengths={1}, longest=1, nlong=0, dups=0, kept=180, tie=50),
    "only_byte": dict(sep_byte=[0, 1, 2, 3], kept=[200] * 4, dups=[0] * 4),
    "digits": dict(digit=DIGITS, kept=[200] * len(DIGITS), dups=[0] * len(DIGITS)),
    "positions": dict(n=POSITION_N, placed=POSITION_RUNS),
    "batch_1": dict(n=BATCH_COUNTS[1]),
    "batch_2": dict(n=BATCH_COUNTS[2]),
    "batch_3": dict(n=BATCH_COUNTS[3], shared_xy=True),
    "batch_4": dict(n=BATCH_COUNTS[4], shared_xy=True),
    "batch_5": dict(n=BATCH_COUNTS[5], shared_xy=True),
    "batch_256": dict(zero_images=[0, 100, 255], full_images=[1, 254], shared_xy=True),
}
