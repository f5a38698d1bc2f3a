"""Python restatement of the global-alignment planner and of the narrow traceback corridor --
TEST INFRASTRUCTURE (tests/test_global_classes.py).

Restated from the code, not from its comments:
  glob_class        bsw_global.hip   class of a job: the int16 bound, then band / column / wide
  cap_dw            bsw_global_k.h   glob_cap_dw: traceback dwords per row of a class's waves
  narrow_tb         bsw_host.cpp     glob_device: a column class takes the kTbEnv-dword window
  path_cells        bsw_global.hip   glob_traceback: the cells the walk reads, rebuilt from a CIGAR
  leaves_corridor   bsw_global.hip   glob_lane_kernel + glob_traceback: the job goes to the retry list

Classes 0..4 are the band kernels (32, 48, 64, 80, 96 slots), 5..9 the column kernels (32, 64,
96, 128, 160 columns), 10 the wide kernel.
"""

BAND_W = (32, 48, 64, 80, 96)            # kGlobBandW
QMAX = (32, 64, 96, 128, 160)            # kGlobQmax
LANE0 = len(BAND_W)                      # kGlobLane0
WIDE = LANE0 + len(QMAX)                 # kGlobWideClass
N_CLASSES = WIDE + 1
MAX_LEN = 1023                           # BSW_MAX_LEN (include/bsw_seqpair.h)
I16_BOUND = 15000                        # glob_class: `bound < 15000` keeps a job on the int16 row
# glob_device (bsw_host.cpp): `constexpr int tb_env = 3` -- the dwords per row a column class keeps
# of the traceback matrix when its full window (cap_dw) is wider than that
TB_ENV = 3


def maxabs(params):
    return max(abs(int(v)) for v in params.mat)


def glob_bound(q, t, params):
    """The planner's bound on every finite cell value (glob_class)."""
    oe_del, oe_ins = params.o_del + params.e_del, params.o_ins + params.e_ins
    return (maxabs(params) * min(q, t) + params.o_del + params.e_del * (t + 1) + params.o_ins +
            params.e_ins * (q + 1) + max(oe_del, oe_ins) + 8)


def glob_class(q, t, w, params, prefer_band):
    if q < 0 or t < 0 or w < 0 or q > MAX_LEN or t > MAX_LEN:
        return -1
    col = -1
    if glob_bound(q, t, params) < I16_BOUND:
        for c, qm in enumerate(QMAX):
            if q <= qm:
                col = c
                break
    need = 2 * w + 2
    band = -1
    for c, bw in enumerate(BAND_W):
        if need <= bw:
            band = c
            break
    if band >= 0 and (col < 0 or prefer_band):
        return band
    return LANE0 + col if col >= 0 else WIDE


def cap_dw(cls, qmax, wmax):
    if cls < LANE0:
        return BAND_W[cls] // 8
    band = ((2 * wmax) >> 3) + 2
    full = QMAX[cls - LANE0] // 8 if cls < WIDE else (qmax + 7) // 8 + 1
    return min(band, full)


def narrow_tb(cls, class_wmax, class_qmax):
    """glob_device: tb = (want && col && tb_env > 0 && tb_env < cap_dw) ? tb_env : 0, for a call that
    asks for CIGARs; class_wmax / class_qmax are the maxima over the class's jobs of the call."""
    return LANE0 <= cls < WIDE and TB_ENV < cap_dw(cls, class_qmax, class_wmax)


def undefined_geometry(qlen, tlen, w):
    """The traceback start lies outside the band: n_cigar = -2, no walk."""
    return qlen >= 1 and tlen >= 1 and qlen < tlen - w


def path_walk(cigar, qlen, tlen, w):
    """-> (cells, (i, k)): the cells (i, k) glob_traceback reads for a job whose CIGAR [(op, len)]
    is `cigar`, and where the walk stops (i < 0 or k < 0).  The walk starts at (tlen - 1,
    min(tlen + w, qlen) - 1), reads one cell per step and then moves by the step's op, taken from
    the CIGAR's end backwards; what is left once a coordinate runs out is pushed in one piece and
    reads nothing."""
    i, k = tlen - 1, min(tlen + w, qlen) - 1
    cells = []
    for op, ln in reversed(cigar):
        for _ in range(ln):
            if i < 0 or k < 0:
                return cells, (i, k)
            cells.append((i, k))
            if op == 0:
                i -= 1
                k -= 1
            elif op == 2:
                i -= 1
            else:
                k -= 1
    return cells, (i, k)


def path_cells(cigar, qlen, tlen, w):
    return path_walk(cigar, qlen, tlen, w)[0]


def _cdiv(a, b):
    """C's integer division (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def corridor(qlen, tlen, tb_dw=TB_ENV):
    """-> (xs, doff) of glob_lane_kernel."""
    dlt = qlen - tlen
    xs = _cdiv(8 * tb_dw - 8 - abs(dlt), 2)
    return xs, min(0, dlt) - xs


def in_window(i, k, doff, tb_dw=TB_ENV):
    """Cell (i, k) lies in the tb_dw dwords row i keeps, from dword max(i + doff, 0) >> 3."""
    return 0 <= (k >> 3) - (max(i + doff, 0) >> 3) < tb_dw


def leaves_corridor(cigar, qlen, tlen, w, tb_dw=TB_ENV):
    """The narrow pass appends the job to the retry list: no room for the corridor (xs < 0) or a
    cell of the walk outside its row's window.  Never for the undefined geometry."""
    if undefined_geometry(qlen, tlen, w):
        return False
    xs, doff = corridor(qlen, tlen, tb_dw)
    if xs < 0:
        return True
    return any(not in_window(i, k, doff, tb_dw) for i, k in path_cells(cigar, qlen, tlen, w))


def unpack_cigar(words, n):
    return [(int(x) & 0xf, int(x) >> 4) for x in words[:n]]


def plan(pairs, params, prefer_band):
    """Per-call prediction from a SeqPair array: (classes per job, {class: (count, wmax, qmax)})."""
    cls = [glob_class(int(p["len2"]), int(p["len1"]), int(p["h0"]), params, prefer_band) for p in pairs]
    st = {}
    for c, p in zip(cls, pairs):
        n, wm, qm = st.get(c, (0, 0, 0))
        st[c] = (n + 1, max(wm, int(p["h0"])), max(qm, int(p["len2"])))
    return cls, st


def predict_retries(pairs, cigar, n_cigar, params, prefer_band):
    """n_tb_retry of a CIGAR call over `pairs` whose oracle CIGARs are (cigar, n_cigar): the jobs of
    the classes on the narrow window that leave their corridor.  -> (count, per-job flags)."""
    cls, st = plan(pairs, params, prefer_band)
    flags = []
    for j, (c, p) in enumerate(zip(cls, pairs)):
        q, t, w = int(p["len2"]), int(p["len1"]), int(p["h0"])
        if not narrow_tb(c, st[c][1], st[c][2]):
            flags.append(False)
        elif undefined_geometry(q, t, w):
            flags.append(False)
        else:
            assert n_cigar[j] >= 0, "the oracle's CIGAR must be complete (stride too small)"
            flags.append(leaves_corridor(unpack_cigar(cigar[j], n_cigar[j]), q, t, w))
    return sum(flags), flags
