"""What tests/test_memchain_edges.py shares: a small two-strand index, hand-built intervals that put a
seed at any (rbeg, qbeg, len), and the three ways a batch is chained -- the C oracle (oracle/chain_ref.c),
the Python transcription (tests/memchain_py.py) and bsw_mem_chain_device.  A plain module, not a test.

The chainer is a pure function of (suffix array, intervals): it never asks whether an interval is a real
SMEM.  So {x[0] = isa[rbeg], x[2] = 1, info = qbeg << 32 | qbeg + len} is a seed at (rbeg, qbeg, len), and a raw
row range {x[0] = row, x[2] = size} is size seeds of one (qbeg, len) at whatever the rows hold."""

import functools

import numpy as np

import bsw
import memchain_py
import oracle

N = 20_000                      # reference bases = l_pac; the text has 2N positions, the suffix array 2N + 1 rows
E_INVAL, E_RANGE = -22, -34


@functools.lru_cache(maxsize=None)
def index():
    """(ref, sa, isa) of the oracle's index of a random reference, read-only"""
    ref = np.random.default_rng(20).integers(0, 4, N, dtype=np.uint8)
    sa = oracle.FmiRef(ref).sa()
    isa = np.zeros(len(sa), np.int64)
    isa[sa] = np.arange(len(sa))
    for a in (ref, sa, isa):
        a.setflags(write=False)
    return ref, sa, isa


def copt(**kw):
    """bwa's defaults with kw over them, as the dict the transcription reads (the floats as C holds them)"""
    o = oracle.chain_opt(**kw)
    return {f: getattr(o, f) for f, _ in o._fields_}


class Batch:
    """reads: per read a list of (rbeg, qbeg, len) seeds or raw (row, size, qbeg, len) intervals, in the order
    the chainer is to see them; lens: the read lengths; counts: n_mems when it is not the number given (a
    value above cap is clamped by the chainer); cap: the interval array's width, else the longest list"""

    def __init__(self, reads, lens, counts=None, cap=None):
        _, sa, isa = index()
        n = len(reads)
        self.n = n
        self.cap = max([len(r) for r in reads] + [0]) if cap is None else cap
        self.mems = np.zeros((n, self.cap), dtype=bsw.BWTINTV_DTYPE)
        self.cnt = np.array([len(r) for r in reads] if counts is None else counts, dtype=np.int32).reshape(n)
        self.lens = (np.full(n, lens, np.int32) if np.isscalar(lens) else np.asarray(lens, np.int32)).reshape(n)
        for r, items in enumerate(reads):
            assert len(items) <= self.cap
            for t, it in enumerate(items):
                if len(it) == 3:
                    rbeg, qbeg, ln = it
                    row, size = int(isa[rbeg]), 1
                else:
                    row, size, qbeg, ln = it
                assert 0 <= row and size >= 1 and row + size <= len(sa) and qbeg >= 0 and ln >= 1
                assert int(sa[row:row + size].max()) + ln <= 2 * N, "a seed past the end of the text"
                self.mems[r, t] = (row, 0, size, (qbeg << 32) | (qbeg + ln))
        self.mems.setflags(write=False)
        self.cnt.setflags(write=False)
        self.lens.setflags(write=False)


def chain_lists(out, n):
    """(seeds, seed_read, seed_chain) -> per read [[(rbeg, qbeg, len), ...] per chain]; the grouping rules of
    include/bsw_fmi.h are asserted on the way: reads ascending, chains 0, 1, ... in runs"""
    seeds, sr, sc = out
    assert len(seeds) == len(sr) == len(sc)
    got = [[] for _ in range(n)]
    for k in range(len(seeds)):
        r, c = int(sr[k]), int(sc[k])
        assert 0 <= r < n and (k == 0 or r >= sr[k - 1]), k
        assert c in (len(got[r]) - 1, len(got[r])), k
        if c == len(got[r]):
            got[r].append([])
        got[r][c].append((int(seeds[k]["rbeg"]), int(seeds[k]["qbeg"]), int(seeds[k]["len"])))
    return got


def same_out(want, got, tag):
    """seed_read, seed_chain, rbeg, qbeg, len exactly"""
    assert len(got[0]) == len(want[0]), f"{tag}: {len(got[0])} seeds, want {len(want[0])}"
    for name, w, g in (("seed_read", want[1], got[1]), ("seed_chain", want[2], got[2])) + \
            tuple((f, want[0][f], got[0][f]) for f in ("rbeg", "qbeg", "len")):
        bad = np.flatnonzero(w != g)
        assert len(bad) == 0, f"{tag}: {name} differs at {len(bad)} seeds, first {bad[:5]} (reads {want[1][bad[:5]]}): " \
                              f"want {w[bad[:5]]} got {g[bad[:5]]}"


def run_oracle(b, **kw):
    return oracle.mem_chain(index()[1], N, b.lens, b.mems, b.cnt, oracle.chain_opt(**kw))


def run_python(b, **kw):
    """the transcription read by read -> chain lists"""
    sa, opt = index()[1], copt(**kw)
    out = []
    for r in range(b.n):
        ms = [(int(m["k"]), int(m["l"]), int(m["s"]), int(m["info"])) for m in b.mems[r, :min(int(b.cnt[r]), b.cap)]]
        out.append(memchain_py.mem_chain_read(opt, sa, N, int(b.lens[r]), ms))
    return out


class Device:
    """a resident bsw.Fmi of the same reference; its suffix array is checked against the oracle's once"""

    def __init__(self, flags=None):
        ref, sa, _ = index()
        self.fmi = bsw.Fmi(ref, flags=flags)
        assert np.array_equal(self.fmi.sa(), sa), "the product's suffix array is not the oracle's"
        self._up = {}

    def close(self):
        self._up.clear()
        self.fmi.close()

    def upload(self, b):
        import hiprt
        if id(b) not in self._up:
            self._up[id(b)] = (b, hiprt.DeviceBuffer.from_array(b.lens), hiprt.DeviceBuffer.from_array(b.mems),
                               hiprt.DeviceBuffer.from_array(b.cnt))
        return self._up[id(b)][1:]

    def call(self, b, seed_cap, bufs=None, **kw):
        """one bsw_mem_chain_device call -> (status, n_seeds); bufs = (d_seeds, d_sr, d_sc) or none"""
        d_len, d_mems, d_cnt = self.upload(b)
        ptrs = [x.ptr for x in bufs] if bufs else [0, 0, 0]
        return self.fmi.mem_chain_device(d_len.ptr, b.n, d_mems.ptr if b.cap else 0, b.cap, d_cnt.ptr, *ptrs, seed_cap,
                                         bsw.chain_opt(**kw))

    def run(self, b, slack=0, **kw):
        """the two-call sizing protocol: seed_cap 0 asks for the count, the second call fills exactly that
        many (+ slack) -> (seeds, seed_read, seed_chain)"""
        import hiprt
        rc, need = self.call(b, 0, **kw)
        assert rc == (E_RANGE if need else 0), (rc, need)
        bufs = (hiprt.DeviceBuffer((need + slack + 1) * bsw.SEED_DTYPE.itemsize), hiprt.DeviceBuffer((need + slack + 1) * 4),
                hiprt.DeviceBuffer((need + slack + 1) * 4))
        rc, got = self.call(b, need + slack, bufs, **kw)
        assert (rc, got) == (0, need), (rc, got, need)
        return (bufs[0].download(np.zeros(need, bsw.SEED_DTYPE)), bufs[1].download(np.zeros(need, np.int32)),
                bufs[2].download(np.zeros(need, np.int32)))


# ---------------------------------------------------------------- an adversary for klib's introsort
def adversary(n):
    """McIlroy's adaptive adversary ("A Killer Adversary for Quicksort", 1999) played against
    memchain_py.introsort on n keys: a key stays undecided ("gas") until a comparison of two undecided keys
    forces one -- the current pivot candidate if it takes part, else the second -- to the next rank.  The ranks it ends
    with are an input on which the median-of-three partitions keep peeling off a few keys, so the depth
    limit runs out and the rest goes to comb sort.  Deterministic: a permutation of 0 .. n - 1."""
    gas = n
    val = [gas] * n
    st = {"solid": 0, "cand": 0}

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            val[x if x == st["cand"] else y] = st["solid"]
            st["solid"] += 1
        if val[x] == gas:
            st["cand"] = x
        elif val[y] == gas:
            st["cand"] = y
        return val[x] < val[y]

    memchain_py.introsort(list(range(n)), lt)
    for i in range(n):
        if val[i] == gas:
            val[i] = st["solid"]
            st["solid"] += 1
    return val
