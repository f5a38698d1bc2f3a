"""Chaining threshold by threshold (csrc/bsw_memchain.hip k_count / k_chain / k_emit; include/bsw_fmi.h
bsw_mem_chain_device): hand-built seeds on every comparison of test_and_merge, mem_chain_weight, mem_chain_flt
and klib's introsort that tests/test_memchain.py's SMEM-derived seeds never land on, and every field of
bsw_chain_opt_t away from its default.  The harness is tests/chainkit.py.

  1. HAND: small reads whose expected chains are literals below, derived from the rules in include/bsw_fmi.h
     (each case's comment carries the arithmetic); oracle, transcription and GPU must all equal them.
  2. the float sweep: mask_level / drop_ratio that are no dyadic fractions, where C's float product and a
     double one fall on different sides of an integer.
  3. the weight sort: chain counts around its 16-element cutoffs with tied weights, and adversary sequences
     that run it out of depth and into comb sort.
  4. scratch sizing: interval sizes 1..40 under max_occ 1..8, every read against its neighbours.
  5. the call contract.

Every batch is chained three ways: the C oracle and the Python transcription on the CPU, the kernel in the
tests marked gpu (seed_read, seed_chain, rbeg, qbeg, len exactly).  The oracle's outputs are computed once
per (batch, options) and shared.  Parity with upstream stays unpinned (no upstream source at hand)."""

import functools

import numpy as np
import pytest

import bsw
import chainkit as ck
import memchain_py
import oracle

gpu = pytest.mark.gpu
L = ck.N                                    # l_pac
RL = 300                                    # read length of the hand cases (any >= min_seed_len: only that is read)
WIDE = bsw.FMI_GPU_BUILD | bsw.FMI_WIDE


@pytest.fixture(scope="module", params=[None, WIDE], ids=["narrow", "wide"])
def dev(request):
    """k_chain<uint32_t> and k_chain<uint64_t>"""
    d = ck.Device(request.param)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev0():
    d = ck.Device()
    yield d
    d.close()


# ================================================================= 1. hand-written expectations
# option sets (bwa's defaults under them: max_occ 500, w 100, max_chain_gap 10000, min_chain_weight 0,
# min_seed_len 19, max_chain_extend 1 << 30, drop_ratio 0.5, mask_level 0.5)
OPTS = {
    "band": dict(w=5, max_chain_gap=40),
    "w0": dict(w=0, max_chain_gap=40),
    "mcw30": dict(w=5, max_chain_gap=40, min_chain_weight=30),
    "mcw31": dict(w=5, max_chain_gap=40, min_chain_weight=31),
    "msl30": dict(min_seed_len=30),
    "mask0": dict(mask_level=0.0),
    "def": dict(),
    "ext0": dict(max_chain_extend=0),
    "ext1": dict(max_chain_extend=1),
    "ext2": dict(max_chain_extend=2),
    "ext3": dict(max_chain_extend=3),
    "ext4": dict(max_chain_extend=4),
}

# Notation of the comments: a seed is (rbeg, qbeg, len); against a chain's last seed, x = qbeg - last.qbeg and
# y = rbeg - last.rbeg; a seed grows the chain when y >= 0, x - y <= w, y - x <= w, x - last.len < max_chain_gap
# and y - last.len < max_chain_gap.  Chains leave in weight order, heaviest first; with two chains a tie keeps
# start order (ks_introsort swaps two elements only when the second is strictly heavier), and no case with
# three or more chains has a tie.  Chains whose query spans do not overlap never shadow one another.
A20 = (1000, 0, 20)
AA = [(1000, 0, 20), (1010, 10, 20)]            # x = y = 10: one chain, query span 0..30, weight 30
CC = [(1000, 10, 20), (1015, 25, 20)]           # x = y = 15: one chain, query 10..45, reference 1000..1035, weight 35
A100, C60 = (1000, 0, 100), (5000, 0, 60)       # C overlaps A by 60 >= 60 * mask: A's first shadowed chain, 60 >= 50: kept
SEC = [A100, (3000, 0, 90), (5000, 0, 80), (7000, 0, 70), (9000, 100, 40)]
# SEC: every chain of query 0.. overlaps every heavier one in full and none is below half of it: kept = 2, and
# each is the first shadowed chain of the one before it: kept = 1 (three secondaries); (9000, 100, 40) starts
# where A100 ends (e_min == b_max: no overlap): kept = 3.  The count loop breaks at the max_chain_extend-th
# secondary and clears it and every later one below 3 -- upstream's quirk: the chain at which it breaks goes too.

HAND = [
    # ---- test_and_merge: the band (w = 5)
    ("x-y == w", "band", [A20, (1022, 27, 20)], [[A20, (1022, 27, 20)]]),                    # x 27, y 22
    ("x-y == w+1", "band", [A20, (1022, 28, 20)], [[A20], [(1022, 28, 20)]]),                # x 28, y 22
    ("y-x == w", "band", [A20, (1027, 22, 20)], [[A20, (1027, 22, 20)]]),                    # x 22, y 27
    ("y-x == w+1", "band", [A20, (1028, 22, 20)], [[A20], [(1028, 22, 20)]]),
    # ---- the gaps (max_chain_gap = 40, last.len = 20)
    ("x-len == gap-1", "band", [A20, (1054, 59, 20)], [[A20, (1054, 59, 20)]]),              # x 59, y 54
    ("x-len == gap", "band", [A20, (1055, 60, 20)], [[A20], [(1055, 60, 20)]]),              # x 60, y 55
    ("y-len == gap-1", "band", [A20, (1059, 54, 20)], [[A20, (1059, 54, 20)]]),              # x 54, y 59
    ("y-len == gap", "band", [A20, (1060, 55, 20)], [[A20], [(1060, 55, 20)]]),              # x 55, y 60
    # ---- y = 0 and y = -1: y is taken from the chain's last seed, which may lie past the chain's start
    ("y == 0 at the start", "band", [A20, (1000, 3, 20)], [[A20, (1000, 3, 20)]]),           # x 3, y 0, not contained
    ("y == 0", "band", AA + [(1010, 13, 20)], [AA + [(1010, 13, 20)]]),                      # x 3, y 0
    # x 2, y -1: a new chain of query 12..32; it overlaps AA's 0..30 by 18 >= 20 * 0.5, 20 >= 30 * 0.5: kept
    ("y == -1", "band", AA + [(1009, 12, 20)], [AA, [(1009, 12, 20)]]),
    # ---- a contained seed is swallowed; one base outside an edge it is not (and y < 0: a new chain of the
    # same weight 35, after CC in start order unless it starts before it; the two overlap, none below half)
    ("contained, flush", "band", CC + [(1000, 10, 35)], [CC]),
    ("contained, inside", "band", CC + [(1005, 20, 10)], [CC]),
    ("query begin - 1", "band", CC + [(1000, 9, 35)], [CC, [(1000, 9, 35)]]),
    ("query end + 1", "band", CC + [(1000, 11, 35)], [CC, [(1000, 11, 35)]]),
    ("ref begin - 1", "band", CC + [(999, 10, 35)], [[(999, 10, 35)], CC]),
    ("ref end + 1", "band", CC + [(1001, 10, 35)], [CC, [(1001, 10, 35)]]),
    # ---- w = 0: the diagonal alone
    ("w0 on the diagonal", "w0", [A20, (1025, 25, 20)], [[A20, (1025, 25, 20)]]),
    ("w0 x-y == 1", "w0", [A20, (1025, 26, 20)], [[A20], [(1025, 26, 20)]]),
    ("w0 y-x == 1", "w0", [A20, (1026, 25, 20)], [[A20], [(1026, 25, 20)]]),
    # ---- strands: l_pac = L
    ("ends at l_pac", "band", [(L - 20, 0, 20)], [[(L - 20, 0, 20)]]),
    ("starts at l_pac", "band", [(L, 0, 20)], [[(L, 0, 20)]]),
    ("straddles l_pac", "band", [(L - 10, 0, 20), (3000, 30, 20)], [[(3000, 30, 20)]]),
    ("one base past l_pac", "band", [(L - 19, 0, 20), (3000, 30, 20)], [[(3000, 30, 20)]]),
    ("one base before l_pac", "band", [(L - 1, 0, 20), (3000, 30, 20)], [[(3000, 30, 20)]]),
    # x = y = 30, gaps 10: in band, but the chain is forward and the seed reverse
    ("forward chain, reverse seed", "band", [(L - 30, 0, 20), (L, 30, 20)], [[(L - 30, 0, 20)], [(L, 30, 20)]]),
    ("reverse chain, reverse seed", "band", [(L, 0, 20), (L + 30, 30, 20)], [[(L, 0, 20), (L + 30, 30, 20)]]),
    # ---- the chain list.  (1022, 22, 21) would grow the chain of (1000, 0, 20) (x = y = 22) but is tried
    # against its lower neighbour (1010, 200, 22) alone (y - x = 190)
    ("nearest lower neighbour only", "band", [A20, (1010, 200, 22), (1022, 22, 21)],
     [[(1010, 200, 22)], [(1022, 22, 21)], [A20]]),
    # equal starts: the list is [q0, q60, q30] (a new chain goes right after the first equal one), so the
    # lower neighbour of rbeg 2001 is q30, which (2001, 31, 25) grows (x = y = 1; weight 21 + 5); appended
    # instead, the list would end with q60 (y - x = 30) and the seed would start a fourth chain
    ("placement after the first equal start", "band", [(2000, 0, 20), (2000, 30, 21), (2000, 60, 22), (2001, 31, 25)],
     [[(2000, 30, 21), (2001, 31, 25)], [(2000, 60, 22)], [(2000, 0, 20)]]),
    # (2000, 33, 23) would grow q30 (x 3, y 0) but is tried against the first equal chain q0 alone (x 33, y 0):
    # a chain of its own, 33..56 against 30..56 of the heavier (26): overlaps, 23 >= 13: kept
    ("first equal chain only", "band", [(2000, 0, 20), (2000, 30, 21), (2000, 60, 22), (2000, 33, 23), (2001, 31, 25)],
     [[(2000, 30, 21), (2001, 31, 25)], [(2000, 33, 23)], [(2000, 60, 22)], [(2000, 0, 20)]]),
    # the same with a seed that would grow q60, the second of the list (x 3, y 0): 63..86 against 60..82 of
    # the lighter (22): overlaps, 22 >= 11.5: kept
    ("first equal chain only, not the second", "band",
     [(2000, 0, 20), (2000, 30, 21), (2000, 60, 22), (2000, 63, 23), (2001, 31, 25)],
     [[(2000, 30, 21), (2001, 31, 25)], [(2000, 63, 23)], [(2000, 60, 22)], [(2000, 0, 20)]]),
    # ---- weight = min(query coverage, reference coverage) = 30 in every case: kept at min_chain_weight 30 ...
    ("query overlap only", "mcw30", [A20, (1020, 15, 15)], [[A20, (1020, 15, 15)]]),         # query 20 + 10, ref 35
    ("ref overlap only", "mcw30", [A20, (1015, 20, 15)], [[A20, (1015, 20, 15)]]),           # query 35, ref 20 + 10
    ("both, query decides", "mcw30", [A20, (1012, 10, 20)], [[A20, (1012, 10, 20)]]),        # query 30, ref 32
    ("both, ref decides", "mcw30", [A20, (1010, 12, 20)], [[A20, (1010, 12, 20)]]),          # query 32, ref 30
    ("light and heavy chain", "mcw30", [(1000, 0, 30), (3000, 50, 31)], [[(3000, 50, 31)], [(1000, 0, 30)]]),
    # ---- ... and gone at 31: reads without output between reads with output
    ("weight == min_chain_weight", "mcw31", [(1000, 0, 31)], [[(1000, 0, 31)]]),
    ("query overlap only", "mcw31", [A20, (1020, 15, 15)], []),
    ("ref overlap only", "mcw31", [A20, (1015, 20, 15)], []),
    ("both, query decides", "mcw31", [A20, (1012, 10, 20)], []),
    ("both, ref decides", "mcw31", [A20, (1010, 12, 20)], []),
    ("light and heavy chain", "mcw31", [(1000, 0, 30), (3000, 50, 31)], [[(3000, 50, 31)]]),
    # ---- the filter.  min_seed_len 30: a chain within A100, below half of it, goes when 100 - w >= 60
    ("w diff == 2*min_seed_len", "msl30", [A100, C60, (9000, 60, 40)], [[A100], [C60]]),
    ("w diff == 2*min_seed_len - 1", "msl30", [A100, C60, (9000, 59, 41)], [[A100], [C60], [(9000, 59, 41)]]),
    # max_chain_gap 40: (5000, 0, 39) is A100's first shadowed chain (dropped, then restored); the third
    # chain (weight 30, x = y = 24 / 25) lies within A100 and goes only while its span is below 40
    ("min_l == gap-1", "band", [A100, (5000, 0, 39), (9000, 50, 15), (9024, 74, 15)], [[A100], [(5000, 0, 39)]]),
    ("min_l == gap", "band", [A100, (5000, 0, 39), (9000, 50, 15), (9025, 75, 15)],
     [[A100], [(5000, 0, 39)], [(9000, 50, 15), (9025, 75, 15)]]),
    # mask_level 0: one base of overlap shadows (1 >= 0); none does not, although 0 >= 0: e_min > b_max comes first
    ("e_min == b_max", "mask0", [A100, C60, (9000, 100, 30)], [[A100], [C60], [(9000, 100, 30)]]),
    ("e_min == b_max + 1", "mask0", [A100, C60, (9000, 99, 30)], [[A100], [C60]]),
    # the first shadowed chain comes back (kept = 1) although 40 < 50 and 100 - 40 >= 38; the next one does not
    ("first is restored", "def", [A100, (9000, 60, 40)], [[A100], [(9000, 60, 40)]]),
    ("second is dropped", "def", [A100, (9000, 60, 40), (12000, 55, 39)], [[A100], [(9000, 60, 40)]]),
    ("three secondaries, no bound", "def", SEC, [[s] for s in SEC]),
    ("max_chain_extend 0", "ext0", SEC, [[SEC[0]], [SEC[4]]]),
    ("max_chain_extend 1", "ext1", SEC, [[SEC[0]], [SEC[4]]]),
    ("max_chain_extend 2", "ext2", SEC, [[SEC[0]], [SEC[1]], [SEC[4]]]),
    ("max_chain_extend 3", "ext3", SEC, [[SEC[0]], [SEC[1]], [SEC[2]], [SEC[4]]]),
    ("max_chain_extend 4", "ext4", SEC, [[s] for s in SEC]),
]

# (name, options, read length, [seeds], n_mems or None, expected): the read length and the interval count
# (n_mems > cap needs a narrow array: clamp_batch below)
EDGE = [
    ("read_len == min_seed_len", "def", 19, [(1000, 0, 19)], None, [[(1000, 0, 19)]]),
    ("read_len == min_seed_len - 1", "def", 18, [(1000, 0, 18)], None, []),
    ("read_len == min_seed_len again", "def", 19, [(3000, 0, 19)], None, [[(3000, 0, 19)]]),
    ("n_mems == 0", "def", RL, [(1000, 0, 20), (3000, 30, 21)], 0, []),
    ("n_mems == 1 of 2", "def", RL, [(1000, 0, 20), (3000, 30, 21)], 1, [[(1000, 0, 20)]]),
]


@functools.lru_cache(maxsize=None)
def hand_batch(key):
    """(batch, expected chain lists, names) of one option set; the EDGE cases ride with "def" (cap stays 5)"""
    cases = [(n, s, None, RL, e) for (n, k, s, e) in HAND if k == key]
    if key == "def":
        cases += [(n, s, c, rl, e) for (n, k, rl, s, c, e) in EDGE]
    counts = [len(s) if c is None else c for (_, s, c, _, _) in cases]
    b = ck.Batch([s for (_, s, _, _, _) in cases], [rl for (_, _, _, rl, _) in cases], counts)
    return b, [[list(c) for c in e] for (*_, e) in cases], [n for (n, *_) in cases]


@functools.lru_cache(maxsize=None)
def hand_oracle(key):
    return ck.run_oracle(hand_batch(key)[0], **OPTS[key])


def test_hand_cases_are_what_they_claim():
    """every option set is used, the reads without output lie between reads with output, and an expected
    seed is a seed that was given"""
    assert {k for (_, k, _, _) in HAND} == set(OPTS)
    exp = hand_batch("mcw31")[1]
    assert exp[0] and exp[-1] and not any(exp[1:-1]), "reads without output between two reads with output"
    for (_, _, seeds, e) in HAND:
        assert {s for c in e for s in c} <= set(seeds)
    print("hand-expected reads:", len(HAND) + len(EDGE) + clamp_batch()[0].n)


@functools.lru_cache(maxsize=None)
def clamp_batch():
    """cap 2: a read whose n_mems says 5 (clamped to the two stored), between a read of none and a full one"""
    reads = [[(5000, 0, 20)], [(1000, 0, 20), (3000, 30, 21)], [(1000, 0, 20), (3000, 30, 21)], [(1000, 0, 22), (3000, 30, 21)]]
    want = [[], [[(3000, 30, 21)], [(1000, 0, 20)]], [[(3000, 30, 21)], [(1000, 0, 20)]], [[(1000, 0, 22)], [(3000, 30, 21)]]]
    return ck.Batch(reads, RL, counts=[0, 5, 2, 1 << 30], cap=2), want


@pytest.mark.parametrize("key", sorted(OPTS))
def test_hand_cases_oracle_and_transcription(key):
    b, want, names = hand_batch(key)
    got_c = ck.chain_lists(hand_oracle(key), b.n)
    got_py = ck.run_python(b, **OPTS[key])
    for r in range(b.n):
        assert got_c[r] == want[r], f"oracle, {key}: {names[r]}"
        assert got_py[r] == want[r], f"transcription, {key}: {names[r]}"


def test_clamped_counts_oracle_and_transcription():
    b, want = clamp_batch()
    assert ck.chain_lists(ck.run_oracle(b), b.n) == want
    assert ck.run_python(b) == want


@gpu
def test_gpu_hand_cases(dev):
    for key in sorted(OPTS):
        b, want, names = hand_batch(key)
        out = dev.run(b, **OPTS[key])
        got = ck.chain_lists(out, b.n)
        for r in range(b.n):
            assert got[r] == want[r], f"{key}: {names[r]}"
        ck.same_out(hand_oracle(key), out, key)


@gpu
def test_gpu_clamped_counts(dev):
    b, want = clamp_batch()
    assert ck.chain_lists(dev.run(b), b.n) == want


# ================================================================= 2. float products
MASKS = (0.1, 0.3, 0.5, 0.7, 0.9)
DROPS = (0.3, 0.5, 0.7, 0.9)


@functools.lru_cache(maxsize=None)
def sweep():
    """1,599 reads of three chains: A100, C60 (A's first shadowed chain, so the next one can really go) and
    B = (9000, 100 - ov, li), li in 19..59 overlapping A by ov in 1..li: min_l = li, and B is shadowed when
    ov >= li * mask_level and dropped when also li < 100 * drop_ratio (100 - li >= 38 throughout)"""
    par = [(li, ov) for li in range(19, 60) for ov in range(1, li + 1)]
    return ck.Batch([[A100, C60, (9000, 100 - ov, li)] for (li, ov) in par], 200), np.array(par)


@functools.lru_cache(maxsize=None)
def sweep_oracle(mask, drop):
    return ck.run_oracle(sweep()[0], mask_level=mask, drop_ratio=drop)


def _separated(mask):
    """the reads whose B-against-A overlap test comes out differently in float and in double"""
    _, par = sweep()
    m32 = np.float32(mask)
    f = par[:, 1].astype(np.float32) >= par[:, 0].astype(np.float32) * m32
    d = par[:, 1].astype(np.float64) >= par[:, 0].astype(np.float64) * np.float64(m32)
    assert f.dtype == d.dtype == bool and (par[:, 0].astype(np.float32) * m32).dtype == np.float32
    return np.flatnonzero(f != d)


@pytest.mark.parametrize("mask", MASKS)
def test_float_sweep_oracle_equals_transcription(mask):
    b, par = sweep()
    for drop in DROPS:
        got = ck.chain_lists(sweep_oracle(mask, drop), b.n)
        want = ck.run_python(b, mask_level=mask, drop_ratio=drop)
        bad = [r for r in range(b.n) if got[r] != want[r]]
        assert not bad, f"mask {mask} drop {drop}: reads {bad[:5]} (li, ov) {par[bad[:5]].tolist()}"
        n = {len(c) for c in got}
        assert n == {2, 3}, f"mask {mask} drop {drop}: chain counts {n}"


def test_float_sweep_separates_float_from_double(monkeypatch):
    """the sweep holds reads on which a double product decides the other way, and there the oracle follows
    the float: the transcription with its float32 taken out (what it was before) gets them wrong"""
    sep = {m: _separated(m) for m in MASKS}
    print("reads separating float from double, by mask_level:", {m: len(v) for m, v in sep.items()})
    assert sum(len(v) for v in sep.values()) >= 1
    assert len(sep[0.5]) == 0, "0.5 is dyadic: every product is exact"
    b, par = sweep()
    flipped = 0
    for m in MASKS:
        if len(sep[m]) == 0:
            continue
        sub = ck.Batch([[A100, C60, (9000, 100 - int(ov), int(li))] for (li, ov) in par[sep[m]]], 200)
        got = ck.chain_lists(ck.run_oracle(sub, mask_level=m), sub.n)
        assert got == ck.run_python(sub, mask_level=m)
        monkeypatch.setattr(memchain_py, "_f32", float)
        dbl = ck.run_python(sub, mask_level=m)
        monkeypatch.undo()
        flipped += sum(g != d for g, d in zip(got, dbl))
    assert flipped >= 1


@gpu
def test_gpu_float_sweep(dev0):
    b, _ = sweep()
    for mask in MASKS:
        for drop in DROPS:
            ck.same_out(sweep_oracle(mask, drop), dev0.run(b, mask_level=mask, drop_ratio=drop), f"mask {mask} drop {drop}")


# ================================================================= 3. the weight sort
COUNTS = (1, 2, 3, 16, 17, 18, 19, 33, 34, 35)
# (chains, ranks per weight): distinct, distinct, tied; and a tied one whose comb sort range (28) passes gap 10
ADVERSARIES = ((48, 1), (64, 1), (64, 2), (50, 2))
KEEP_ALL = dict(drop_ratio=0.01)                        # nothing is below 1% of another: the output order is the sort's


def _sort_read(weights):
    """chain i = one seed (200 i + 100, 0, w_i): all start at query 0, so all overlap, none merges"""
    return [(200 * i + 100, 0, int(w)) for i, w in enumerate(weights)]


@functools.lru_cache(maxsize=None)
def adversary_weights(n, div):
    return tuple(150 - k // div for k in ck.adversary(n))


@functools.lru_cache(maxsize=None)
def sort_batch():
    """8 draws of three weights per chain count, then the adversary sequences; 151-base reads"""
    rng = np.random.default_rng(35)
    reads = [_sort_read(rng.choice([40, 50, 60], n)) for n in COUNTS for _ in range(8)]
    reads += [_sort_read(adversary_weights(n, div)) for (n, div) in ADVERSARIES]
    return ck.Batch(reads, 151)


@functools.lru_cache(maxsize=None)
def sort_oracle(default_drop):
    return ck.run_oracle(sort_batch(), **({} if default_drop else KEEP_ALL))


def test_adversary_reaches_comb_sort(monkeypatch):
    """the adversary's weights send memchain_py.introsort (hence klib's) into ks_combsort on more than the
    16 elements the final insertion sort would have handled anyway"""
    ranges = []
    real = memchain_py._combsort

    def counting(a, s, n, lt):
        ranges.append(n)
        return real(a, s, n, lt)

    for (n, div) in ADVERSARIES:
        w = adversary_weights(n, div)
        assert len(w) == n and len(set(w)) == (n if div == 1 else n // div) and min(w) >= 19 and max(w) <= 151
    monkeypatch.setattr(memchain_py, "_combsort", counting)
    reached = {}
    for (n, div) in ADVERSARIES:
        del ranges[:]
        got = ck.run_python(ck.Batch([_sort_read(adversary_weights(n, div))], 151), **KEEP_ALL)
        assert len(got[0]) == n
        reached[(n, div)] = list(ranges)
        assert ranges and max(ranges) > 16, (n, div, ranges)
    print("comb sort ranges:", reached)


@pytest.mark.parametrize("default_drop", [False, True], ids=["keep_all", "default_drop"])
def test_sort_oracle_equals_transcription(default_drop):
    b = sort_batch()
    got = ck.chain_lists(sort_oracle(default_drop), b.n)
    want = ck.run_python(b, **({} if default_drop else KEEP_ALL))
    for r in range(b.n):
        assert got[r] == want[r], r
        given = [int(m["info"] & np.uint64(0xffffffff)) for m in b.mems[r, :b.cnt[r]]]      # qbeg 0: info's low half = len
        ws = [c[0][2] for c in got[r]]
        assert sorted(ws, reverse=True) == ws and sorted(ws) == sorted(given), r             # a sorted permutation: all kept
    assert {len(c) for c in got} == set(COUNTS) | {n for (n, _) in ADVERSARIES}


@gpu
def test_gpu_sort(dev):
    b = sort_batch()
    ck.same_out(sort_oracle(False), dev.run(b, **KEEP_ALL), "keep all")
    ck.same_out(sort_oracle(True), dev.run(b), "default drop_ratio")


# ================================================================= 4. scratch sizing
@functools.lru_cache(maxsize=None)
def occ_batch():
    """read s (1..40): row ranges of s, 41 - s and (7 s) % 40 + 1 rows (k_count sizes the read's scratch region
    as min(max_occ, ceil(size / step)) per interval, k_chain fills it: one seed too few and a read writes
    into the next one's region); the rows hold whatever the suffix array does, away from the text's end"""
    _, sa, _ = ck.index()
    rng = np.random.default_rng(40)
    reads = []
    for s in range(1, 41):
        items = []
        for t, size in enumerate((s, 41 - s, (7 * s) % 40 + 1)):
            while True:
                row = int(rng.integers(1, len(sa) - size))
                if sa[row:row + size].max() + 30 <= 2 * ck.N:
                    break
            items.append((row, size, 45 * t, 19 + (s + t) % 12))
        reads.append(items)
    return ck.Batch(reads, 151)


@functools.lru_cache(maxsize=None)
def occ_oracle(max_occ):
    return ck.run_oracle(occ_batch(), max_occ=max_occ)


def _n_taken(size, max_occ):
    step = size // max_occ if size > max_occ else 1
    return min(max_occ, -(-size // step))


@pytest.mark.parametrize("max_occ", range(1, 9))
def test_occ_sampling_oracle_equals_transcription(max_occ):
    b = occ_batch()
    got = ck.chain_lists(occ_oracle(max_occ), b.n)
    assert got == ck.run_python(b, max_occ=max_occ)
    # the rows sampled are what k_count must count; random positions seldom merge, nest or bridge l_pac, so
    # nearly all of them leave as seeds
    sizes = b.mems["s"].astype(np.int64)
    taken = sum(_n_taken(int(v), max_occ) for v in sizes.reshape(-1))
    assert 0.9 * taken <= len(occ_oracle(max_occ)[0]) <= taken
    assert sorted(np.unique(sizes[:, 0])) == list(range(1, 41))


@gpu
def test_gpu_occ_sampling_sizes_every_region(dev):
    b = occ_batch()
    for max_occ in range(1, 9):
        ck.same_out(occ_oracle(max_occ), dev.run(b, max_occ=max_occ), f"max_occ {max_occ}")


# ================================================================= 5. the call contract
@gpu
def test_gpu_call_contract(dev0):
    import hiprt
    b = sort_batch()
    want = sort_oracle(True)
    total = len(want[0])
    bufs = (hiprt.DeviceBuffer(total * bsw.SEED_DTYPE.itemsize), hiprt.DeviceBuffer(total * 4), hiprt.DeviceBuffer(total * 4))
    assert dev0.call(b, total - 1, bufs) == (ck.E_RANGE, total)
    assert dev0.call(b, total, bufs) == (0, total)
    got = (bufs[0].download(np.zeros(total, bsw.SEED_DTYPE)), bufs[1].download(np.zeros(total, np.int32)),
           bufs[2].download(np.zeros(total, np.int32)))
    ck.same_out(want, got, "seed_cap == total")
    for bad in (dict(max_occ=0), dict(w=-1), dict(max_chain_gap=-1), dict(max_chain_extend=-1)):
        assert dev0.call(b, total, bufs, **bad) == (ck.E_INVAL, 0), bad
    # no reads: nothing is read, not even the pointers
    assert dev0.fmi.mem_chain_device(0, 0, 0, 0, 0, 0, 0, 0, 0) == (0, 0)
    # cap == 0: no intervals whatever n_mems says, d_mems may be null
    none = ck.Batch([[], [], []], 151, counts=[0, 3, 1 << 30], cap=0)
    assert dev0.call(none, 0) == (0, 0)
    assert dev0.call(none, total, bufs) == (0, 0)
    assert len(oracle.mem_chain(ck.index()[1], ck.N, none.lens, none.mems, none.cnt)[0]) == 0
