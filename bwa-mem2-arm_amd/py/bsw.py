"""ctypes binding of the product C ABI (include/bsw.h -> lib/libbsw_hip.so) and of the
synthetic-batch tool (lib/libbsw_synth.so).

This is plumbing for tests and bench.py: the product is the C ABI / C++ shim; PyTorch
is used only for device memory, streams and torch.distributed.  Loading fails loudly
when the HIP library is missing -- there is no CPU fallback anywhere in this module.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(PKG, "lib")
HIP_LIB = os.environ.get("BSW_HIP_LIB") or os.path.join(LIBDIR, "libbsw_hip.so")   # override: experiment builds
SYNTH_LIB = os.environ.get("BSW_SYNTH_LIB") or os.path.join(LIBDIR, "libbsw_synth.so")   # override: `make asan-suite`

SEQPAIR_DTYPE = np.dtype(
    [(n, "<i4") for n in ("idr", "idq", "id", "len1", "len2", "h0", "seqid", "regid",
                          "score", "tle", "gtle", "qle", "gscore", "max_off")]
)
OUT_FIELDS = ("score", "tle", "gtle", "qle", "gscore", "max_off")
assert SEQPAIR_DTYPE.itemsize == 56

# Every symbol include/bsw.h declares (tests check the library exports all of them).
ABI_SYMBOLS = ("bsw_params_default", "bsw_create", "bsw_create_on", "bsw_destroy", "bsw_get_scores",
               "bsw_get_scores_device", "bsw_last_stats", "bsw_strerror", "bsw_abi_version",
               "bsw_pack_batch", "bsw_get_scores_packed_device",
               "bsw_ext_opt_default", "bsw_extend_seeds", "bsw_ext_last_stats",
               "bswb_write", "bswb_read_header", "bswb_read",
               "bsw_ksw_align2", "bsw_ksw_align2_device", "bsw_mate_last_stats",
               "bsw_ksw_global2", "bsw_ksw_global2_device", "bsw_global_last_stats",
               "bsw_set_reference", "bsw_extend_seeds_device", "bsw_set_option",
               "bsw_split_by_cells", "bsw_chain2aln", "bsw_chain2aln_device", "bsw_chain_last_stats",
               "bsw_chain2aln_resident", "bsw_mem_opt_default", "bsw_fmi_build", "bsw_fmi_destroy", "bsw_fmi_get_info", "bsw_fmi_copy_sa",
               "bsw_fmi_copy_bwt", "bsw_mem_collect_intv", "bsw_mem_collect_intv_device", "bsw_fmi_sa_device",
               "bsw_fmi_last_kernel_ms", "bsw_chain_opt_default", "bsw_mem_chain_device", "bsw_fmi_build2", "bsw_fmi_check")

# include/bsw_aln.h (additive to ABI version 8: its functions are listed here, not in ABI_SYMBOLS)
ALN_SYMBOLS = ("bsw_reg2aln", "bsw_reg2aln_resident", "bsw_aln_last_stats")
# include/bsw_sel.h (additive in the same way)
SEL_SYMBOLS = ("bsw_sel_opt_default", "bsw_regs_select", "bsw_regs_select_resident", "bsw_sel_last_stats")
# include/bsw_pe.h (additive in the same way)
PE_SYMBOLS = ("bsw_pe_opt_default", "bsw_pe_stat", "bsw_pe_stat_resident", "bsw_pe_pair", "bsw_pe_pair_resident",
              "bsw_pe_last_stats")
# include/bsw_matesw.h (additive to ABI 8: BSW_MATESW_API)
MATESW_SYMBOLS = ("bsw_matesw_opt_default", "bsw_matesw", "bsw_matesw_resident", "bsw_matesw_last_stats")
# include/bsw_rec.h (additive to ABI 8: BSW_REC_API)
REC_SYMBOLS = ("bsw_rec_opt_default", "bsw_records", "bsw_records_resident", "bsw_sam_text", "bsw_sam_text_resident",
               "bsw_rec_last_stats")
# include/bsw_contigs.h (additive to ABI 8: BSW_CONTIGS_API)
CONTIGS_SYMBOLS = ("bsw_set_contigs", "bsw_fmi_set_contigs")
# include/bsw_bam.h (additive likewise)
BAM_SYMBOLS = ("bsw_bam_records", "bsw_bam_records_resident", "bsw_bam_header", "bsw_bam_last_stats")
# include/bsw_bgzf.h (additive likewise: BSW_BGZF_API)
BGZF_SYMBOLS = ("bsw_bgzf_opt_default", "bsw_bgzf", "bsw_bgzf_resident", "bsw_bgzf_last_stats")
BGZF_MAX_BLOCK, BGZF_EOF = 0xff00, 1
# include/bsw_bamsort.h (additive likewise: BSW_BAMSORT_API)
BAMSORT_SYMBOLS = ("bsw_bam_sort", "bsw_bam_sort_resident", "bsw_bam_index", "bsw_bam_index_resident",
                   "bsw_bamsort_last_stats")
# include/bsw_fmi_launch.h (additive likewise: BSW_FMI_LAUNCH_API)
FMI_LAUNCH_SYMBOLS = ("bsw_fmi_last_launch",)
# include/bsw_markdup.h (additive likewise: BSW_MARKDUP_API)
MARKDUP_SYMBOLS = ("bsw_markdup_opt_default", "bsw_mark_duplicates", "bsw_mark_duplicates_resident", "bsw_markdup_last_stats")
BSW_DUP_PAIR, BSW_DUP_FRAG, BSW_DUP_FRAG_BY_PAIR = 1, 2, 3
MARKDUP_ROUTE_NONE, MARKDUP_ROUTE_ONE, MARKDUP_ROUTE_MULTI = 0, 1, 2
BAMSORT_PERM_TILE = 8192           # bytes of output per workgroup of the permute kernel (bsw_bamsort_k.h: kPermTile), for tests
BAMSORT_SORT_TILE = 4096            # a size above which the radix sort runs over more than one of its tiles, for tests
CONTIG_MAX_NAME = 63

# include/bsw.h engine options (bsw_set_option)
OPT_KERNEL8, OPT_FORK, OPT_SORTKEY, OPT_GLOB_BAND, OPT_EXT_CHUNK, OPT_HOST_CHUNK, OPT_LONG, OPT_HOST_PACK = 1, 2, 3, 4, 5, 6, 7, 8
OPT_SMALL_BATCH = 9
OPT_SPLIT_MIN = 10
OPT_COALESCE = 11
OPT_COALESCE_LEADERS = 12
OPT_GROUP_KERNEL = 13
OPT_MID_BATCH = 14
OPT_COALESCE_LINGER = 16
OPT_GQ32_MAX = 18
OPT_TEST_MISROUTE = 100
OPT_TEST_FAIL_ALLOC = 101

# include/bsw_ext.h structs
SEED_DTYPE = np.dtype([("rbeg", np.int64), ("qbeg", np.int32), ("len", np.int32)])
ALNREG_DTYPE = np.dtype([("rb", np.int64), ("re", np.int64), ("qb", np.int32), ("qe", np.int32),
                         ("score", np.int32), ("truesc", np.int32), ("w", np.int32),
                         ("seedlen0", np.int32)])
assert SEED_DTYPE.itemsize == 16 and ALNREG_DTYPE.itemsize == 40

# include/bsw_aln.h
ALN_DTYPE = np.dtype([("pos", np.int64), ("is_rev", np.int32), ("n_cigar", np.int32), ("NM", np.int32),
                      ("score", np.int32), ("w", np.int32), ("n_pass", np.int32), ("md_len", np.int32),
                      ("flags", np.int32)])
assert ALN_DTYPE.itemsize == 40
ALN_REJECTED, ALN_NODP, ALN_OVERFLOW = 1, 2, 4
# include/bsw_sel.h
SELINFO_DTYPE = np.dtype([("seedcov", np.int32), ("sub", np.int32), ("csub", np.int32), ("sub_n", np.int32),
                          ("n_comp", np.int32), ("secondary", np.int32), ("mapq", np.int32), ("src", np.int32),
                          ("frac_rep", np.float32)])
assert SELINFO_DTYPE.itemsize == 36
# include/bsw_pe.h
PESTAT_DTYPE = np.dtype([("low", np.int32), ("high", np.int32), ("failed", np.int32), ("n", np.int32),
                         ("avg", np.float64), ("std", np.float64)])
PAIR_DTYPE = np.dtype([("paired", np.int32), ("z", np.int32, (2,)), ("mapq", np.int32, (2,)), ("proper", np.int32),
                       ("score", np.int32), ("sub", np.int32), ("n_sub", np.int32), ("q_pe", np.int32)])
assert PESTAT_DTYPE.itemsize == 32 and PAIR_DTYPE.itemsize == 40
PE_MAX_INS = 1 << 16
# include/bsw_rec.h
REC_DTYPE = np.dtype([("pos", np.int64), ("mpos", np.int64), ("tlen", np.int64), ("read", np.int32), ("reg", np.int32),
                      ("aln", np.int32), ("which", np.int32), ("n_list", np.int32), ("flag", np.int32),
                      ("sam_flag", np.int32), ("is_rev", np.int32), ("mapq", np.int32), ("score", np.int32),
                      ("sub", np.int32), ("m_is_rev", np.int32), ("m_aln", np.int32), ("xa_first", np.int32),
                      ("xa_n", np.int32), ("reserved", np.int32)])
assert REC_DTYPE.itemsize == 88
REC_SOFTCLIP, REC_NO_MULTI, REC_KEEP_SUPP_MAPQ = 1, 2, 4

# include/bsw_mate.h
KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000
KSWR_DTYPE = np.dtype([(n, "<i4") for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")])
assert KSWR_DTYPE.itemsize == 28


class Params(ctypes.Structure):
    """Mirror of bsw_params_t (include/bsw.h)."""
    _fields_ = [("o_del", ctypes.c_int32), ("e_del", ctypes.c_int32),
                ("o_ins", ctypes.c_int32), ("e_ins", ctypes.c_int32),
                ("zdrop", ctypes.c_int32), ("end_bonus", ctypes.c_int32),
                ("mat", ctypes.c_int8 * 25), ("w_match", ctypes.c_int8),
                ("w_mismatch", ctypes.c_int8), ("w_ambig", ctypes.c_int8)]


class Stats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_float), ("n_i16", ctypes.c_int32),
                ("n_u8", ctypes.c_int32), ("n_wide", ctypes.c_int32),
                ("n_launches", ctypes.c_int32), ("n_packed", ctypes.c_int32),
                ("stage_ms", ctypes.c_float), ("host_ms", ctypes.c_float), ("n_wave", ctypes.c_int32),
                ("n_devices", ctypes.c_int32), ("n_group", ctypes.c_int32),
                ("recovery", ctypes.c_int32)]


def default_params(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, zdrop=100, end_bonus=5,
                   ambig=-1, mat=None) -> Params:
    p = Params()
    p.o_del, p.e_del, p.o_ins, p.e_ins = o_del, e_del, o_ins, e_ins
    p.zdrop, p.end_bonus = zdrop, end_bonus
    if mat is None:
        mat = [ambig if (t == 4 or q == 4) else (a if t == q else -b)
               for t in range(5) for q in range(5)]
    for i, v in enumerate(mat):
        p.mat[i] = int(v)
    p.w_match, p.w_mismatch, p.w_ambig = a, -b, ambig
    return p


class BswError(RuntimeError):
    pass


_hip = None


def hip_lib():
    """Load libbsw_hip.so (raises if it was not built: no silent fallback)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise BswError(f"{HIP_LIB} not built: run `make` or __graft_entry__.build()")
        L = ctypes.CDLL(HIP_LIB)
        P = ctypes.c_void_p
        L.bsw_params_default.argtypes = [P]
        L.bsw_create.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
        L.bsw_create_on.argtypes = [P, P, ctypes.c_int, ctypes.POINTER(P)]
        L.bsw_destroy.argtypes = [P]
        L.bsw_get_scores.argtypes = [P, P, P, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int]
        L.bsw_get_scores_device.argtypes = [P, P, P, P, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_int, P]
        L.bsw_last_stats.argtypes = [P, P]
        L.bsw_strerror.restype = ctypes.c_char_p
        L.bsw_strerror.argtypes = [ctypes.c_int]
        L.bswb_write.argtypes = [ctypes.c_char_p, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, P,
                                 ctypes.c_int64, P, ctypes.c_int64, P, ctypes.c_int64]
        L.bswb_read_header.argtypes = [ctypes.c_char_p, P]
        L.bswb_read.argtypes = [ctypes.c_char_p, P, P, P, P]
        L.bsw_ext_opt_default.argtypes = [P]
        L.bsw_extend_seeds.argtypes = [P, P, P, ctypes.c_int64, P, P, P, P, ctypes.c_int32, P]
        L.bsw_ext_last_stats.argtypes = [P, P]
        L.bsw_ksw_align2.argtypes = [P, P, P, P, ctypes.c_int32, P]
        L.bsw_ksw_align2_device.argtypes = [P, P, P, P, ctypes.c_int32, P, P]
        L.bsw_mate_last_stats.argtypes = [P, P]
        L.bsw_ksw_global2.argtypes = [P, P, P, P, ctypes.c_int32, P, ctypes.c_int32, P]
        L.bsw_ksw_global2_device.argtypes = [P, P, P, P, ctypes.c_int32, P, ctypes.c_int32, P, P]
        L.bsw_global_last_stats.argtypes = [P, P]
        L.bsw_set_reference.argtypes = [P, P, ctypes.c_int64]
        L.bsw_extend_seeds_device.argtypes = [P, P, P, P, P, P, ctypes.c_int32, P, P]
        L.bsw_set_option.argtypes = [P, ctypes.c_int, ctypes.c_int64]
        L.bsw_split_by_cells.argtypes = [P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P]
        L.bsw_chain2aln.argtypes = [P, P, P, ctypes.c_int64, P, P, P, ctypes.c_int32, P, P, P, ctypes.c_int32, P, P]
        L.bsw_chain2aln_device.argtypes = [P, P, P, P, P, ctypes.c_int32, P, P, P, ctypes.c_int32, P, P]
        L.bsw_chain_last_stats.argtypes = [P, P]
        L.bsw_chain2aln_resident.argtypes = [P, P, P, P, P, ctypes.c_int32, P, P, P, ctypes.c_int32, P, P]
        L.bsw_chain2aln_resident.restype = ctypes.c_int
        L.bsw_mem_opt_default.argtypes = [P]
        L.bsw_fmi_build.argtypes = [P, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(P)]
        L.bsw_fmi_build2.argtypes = [P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
        L.bsw_fmi_build2.restype = ctypes.c_int
        L.bsw_fmi_check.argtypes = [P, P]
        L.bsw_fmi_check.restype = ctypes.c_int
        L.bsw_fmi_destroy.argtypes = [P]
        L.bsw_fmi_get_info.argtypes = [P, P]
        L.bsw_fmi_copy_sa.argtypes = [P, P]
        L.bsw_fmi_copy_bwt.argtypes = [P, P]
        L.bsw_mem_collect_intv.argtypes = [P, P, P, P, P, ctypes.c_int32, P, ctypes.c_int32, P]
        L.bsw_mem_collect_intv_device.argtypes = [P, P, P, P, P, ctypes.c_int32, ctypes.c_int32, P, ctypes.c_int32,
                                                  P, P]
        L.bsw_fmi_sa_device.argtypes = [P, P, ctypes.c_int64, P, P]
        L.bsw_fmi_last_kernel_ms.argtypes = [P, P]
        L.bsw_chain_opt_default.argtypes = [P]
        L.bsw_mem_chain_device.argtypes = [P, P, P, ctypes.c_int32, P, ctypes.c_int32, P, P, P, P, ctypes.c_int64,
                                           P, P]
        L.bsw_mem_chain_device.restype = ctypes.c_int
        L.bsw_pack_batch.argtypes = [P, P, P, ctypes.c_int32, P, ctypes.c_int64, P]
        L.bsw_reg2aln.argtypes = [P, P, P, P, P, ctypes.c_int32, P, P, ctypes.c_int32, P, P, ctypes.c_int32, P,
                                  ctypes.c_int32]
        L.bsw_reg2aln_resident.argtypes = [P, P, P, P, P, ctypes.c_int32, P, P, ctypes.c_int32, P, P, ctypes.c_int32,
                                           P, ctypes.c_int32, P]
        L.bsw_aln_last_stats.argtypes = [P, P]
        for f in ALN_SYMBOLS:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_sel_opt_default.argtypes = [P]
        L.bsw_sel_opt_default.restype = None
        L.bsw_regs_select.argtypes = [P, P, P, P, P, ctypes.c_int32, P, P, P, P, P, ctypes.c_int32, P, P, P, P, P, P,
                                      ctypes.c_int32, P]
        L.bsw_regs_select_resident.argtypes = L.bsw_regs_select.argtypes + [P]
        L.bsw_sel_last_stats.argtypes = [P, P]
        for f in SEL_SYMBOLS[1:]:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_pe_opt_default.argtypes = [P]
        L.bsw_pe_opt_default.restype = None
        L.bsw_pe_stat.argtypes = [P, P, P, P, P, ctypes.c_int32, P]
        L.bsw_pe_stat_resident.argtypes = [P, P, P, P, P, ctypes.c_int32, ctypes.c_int32, P, P]
        L.bsw_pe_pair.argtypes = [P, P, P, P, P, P, ctypes.c_int32, P]
        L.bsw_pe_pair_resident.argtypes = [P, P, P, P, P, P, ctypes.c_int32, ctypes.c_int32, P, P]
        L.bsw_pe_last_stats.argtypes = [P, P]
        for f in PE_SYMBOLS[1:]:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_matesw_opt_default.argtypes = [P]
        L.bsw_matesw_opt_default.restype = None
        L.bsw_matesw.argtypes = [P, P, P, P, P, P, ctypes.c_int32, P, P, P, P, P, P, P, ctypes.c_int32, P]
        L.bsw_matesw_resident.argtypes = [P, P, P, P, P, P, ctypes.c_int32, P, P, P, ctypes.c_int32, P, P, P, P,
                                          ctypes.c_int32, P, P]
        L.bsw_matesw_last_stats.argtypes = [P, P]
        for f in MATESW_SYMBOLS[1:]:
            getattr(L, f).restype = ctypes.c_int
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        L.bsw_rec_opt_default.argtypes = [P]
        L.bsw_rec_opt_default.restype = None
        L.bsw_records.argtypes = [P, P, P, P, P, i32, P, P, P, P, P, P, i32, P, P, P, i32, P, i32, i32, P, P]
        L.bsw_records_resident.argtypes = [P, P, P, P, P, i32, P, P, P, i32, P, P, P, i32, P, P, P, i32, P, i32, i32, P, P,
                                           P]
        L.bsw_sam_text.argtypes = [P, P, P, P, i32, P, P, i32, P, i32, i32, P, P, P, i32, P, P, P, i32, P, P, i64, P]
        L.bsw_sam_text_resident.argtypes = L.bsw_sam_text.argtypes + [P]
        L.bsw_rec_last_stats.argtypes = [P, P]
        for f in REC_SYMBOLS[1:]:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_bam_records.argtypes = L.bsw_sam_text.argtypes
        L.bsw_bam_records_resident.argtypes = L.bsw_sam_text_resident.argtypes
        L.bsw_bam_header.argtypes = [P, P, P, i32, P, i64, P]
        L.bsw_bam_last_stats.argtypes = [P, P]
        for f in BAM_SYMBOLS:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_bgzf_opt_default.argtypes = [P]
        L.bsw_bgzf_opt_default.restype = None
        L.bsw_bgzf.argtypes = [P, P, P, i64, P, i32, P, i64, P, i32, P, P, P]
        L.bsw_bgzf_resident.argtypes = L.bsw_bgzf.argtypes + [P]
        L.bsw_bgzf_last_stats.argtypes = [P, P]
        for f in BGZF_SYMBOLS[1:]:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_bam_sort.argtypes = [P, P, P, P, i32, P, i64, P, P]
        L.bsw_bam_sort_resident.argtypes = L.bsw_bam_sort.argtypes + [P]
        L.bsw_bam_index.argtypes = [P, P, P, P, P, i32, P, i64, P, i64, P]
        L.bsw_bam_index_resident.argtypes = L.bsw_bam_index.argtypes + [P]
        L.bsw_bamsort_last_stats.argtypes = [P, P]
        for f in BAMSORT_SYMBOLS:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_markdup_opt_default.argtypes = [P]
        L.bsw_markdup_opt_default.restype = None
        L.bsw_mark_duplicates.argtypes = [P, P, P, P, i32, P, P, i32, i32, P, P, i32, P, i64, i32, P]
        L.bsw_mark_duplicates_resident.argtypes = L.bsw_mark_duplicates.argtypes + [P]
        L.bsw_markdup_last_stats.argtypes = [P, P]
        for f in MARKDUP_SYMBOLS[1:]:
            getattr(L, f).restype = ctypes.c_int
        L.bsw_set_contigs.argtypes = [P, i32, P, ctypes.POINTER(ctypes.c_char_p)]
        L.bsw_set_contigs.restype = ctypes.c_int
        L.bsw_fmi_set_contigs.argtypes = [P, i32, P]
        L.bsw_fmi_set_contigs.restype = ctypes.c_int
        L.bsw_fmi_last_launch.argtypes = [P, P, P]
        L.bsw_fmi_last_launch.restype = ctypes.c_int
        L.bsw_get_scores_packed_device.argtypes = [P, P, P, ctypes.c_int32, ctypes.c_int, P, P]
        if hasattr(L, "bsw_sort_order_device"):     # test hook, no part of the ABI (an older experiment build lacks it)
            L.bsw_sort_order_device.argtypes = [P, P, ctypes.c_int32, ctypes.c_int, ctypes.c_int, P]
            L.bsw_sort_order_device.restype = ctypes.c_int
        for f in ("bsw_create", "bsw_create_on", "bsw_get_scores", "bsw_get_scores_device", "bsw_last_stats",
                  "bsw_pack_batch", "bsw_get_scores_packed_device",
                  "bsw_abi_version", "bsw_extend_seeds", "bsw_ext_last_stats", "bswb_write",
                  "bswb_read_header", "bswb_read", "bsw_ksw_align2", "bsw_ksw_align2_device",
                  "bsw_mate_last_stats", "bsw_ksw_global2", "bsw_ksw_global2_device", "bsw_global_last_stats",
                  "bsw_set_reference", "bsw_extend_seeds_device", "bsw_set_option",
               "bsw_split_by_cells", "bsw_chain2aln", "bsw_chain2aln_device", "bsw_chain_last_stats",
                  "bsw_fmi_build", "bsw_fmi_get_info", "bsw_fmi_copy_sa", "bsw_fmi_copy_bwt", "bsw_mem_collect_intv",
                  "bsw_mem_collect_intv_device", "bsw_fmi_sa_device", "bsw_fmi_last_kernel_ms"):
            getattr(L, f).restype = ctypes.c_int
        _hip = L
    return _hip


def _check(rc):
    if rc != 0:
        raise BswError(f"bsw error {rc}: {hip_lib().bsw_strerror(rc).decode()}")


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


class Engine:
    """Python mirror of the C++ shim: one engine = one bsw_ctx_t."""

    def __init__(self, params: Params | None = None, device: int = 0, n_gpus: int = 1,
                 devices: list[int] | None = None, **options):
        """devices: explicit logical-device -> HIP-device map (bsw_create_on; repeats allowed,
        the rehearsal of an n-GPU context on a smaller box); else devices [device, device + n_gpus)."""
        self.params = params if params is not None else default_params()
        self._ctx = ctypes.c_void_p()
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices)
            _check(hip_lib().bsw_create_on(ctypes.byref(self.params), arr, len(devices), ctypes.byref(self._ctx)))
        else:
            _check(hip_lib().bsw_create(ctypes.byref(self.params), device, n_gpus, ctypes.byref(self._ctx)))
        for k, v in options.items():
            self.set_option(k, v)

    _OPTS = {"kernel8": OPT_KERNEL8, "fork": OPT_FORK, "sortkey": OPT_SORTKEY, "glob_band": OPT_GLOB_BAND,
             "ext_chunk": OPT_EXT_CHUNK, "host_chunk": OPT_HOST_CHUNK, "long": OPT_LONG, "host_pack": OPT_HOST_PACK,
             "small_batch": OPT_SMALL_BATCH, "split_min": OPT_SPLIT_MIN, "coalesce": OPT_COALESCE, "coalesce_leaders": OPT_COALESCE_LEADERS, "group_kernel": OPT_GROUP_KERNEL, "mid_batch": OPT_MID_BATCH,
             "coalesce_linger": OPT_COALESCE_LINGER, "gq32_max": OPT_GQ32_MAX,
             "test_misroute": OPT_TEST_MISROUTE, "test_fail_alloc": OPT_TEST_FAIL_ALLOC}

    def set_option(self, name, value: int):
        """bsw_set_option by name (kernel8, fork, sortkey, glob_band, ext_chunk, host_chunk, test_misroute)
        or by BSW_OPT_* number."""
        opt = self._OPTS[name] if isinstance(name, str) else int(name)
        _check(hip_lib().bsw_set_option(self._ctx, opt, int(value)))

    def close(self):
        if self._ctx:
            hip_lib().bsw_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_scores(self, pairs: np.ndarray, ref: np.ndarray, qer: np.ndarray, w: int,
                   cell_bits: int = 16):
        """getScores16 / getScores8 on host buffers; results in place in `pairs`."""
        assert pairs.dtype == SEQPAIR_DTYPE and pairs.flags.c_contiguous
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        qer = np.ascontiguousarray(qer, dtype=np.uint8)
        _check(hip_lib().bsw_get_scores(self._ctx, _ptr(pairs), _ptr(ref), _ptr(qer),
                                        len(pairs), w, cell_bits))

    def get_scores_device(self, d_pairs: int, d_ref: int, d_qer: int, n: int, w: int,
                          cell_bits: int = 16, stream: int = 0):
        """Device-resident call: raw device pointers (e.g. torch tensor .data_ptr())."""
        _check(hip_lib().bsw_get_scores_device(self._ctx, ctypes.c_void_p(d_pairs),
                                               ctypes.c_void_p(d_ref), ctypes.c_void_p(d_qer),
                                               n, w, cell_bits, ctypes.c_void_p(stream)))

    def get_scores_packed_device(self, d_packed: int, desc: "Packed", w: int, cell_bits: int, d_out: int,
                                 stream: int = 0):
        """bsw_get_scores_packed_device: a packed batch (bsw_pack_batch) resident at d_packed;
        the 6 output int32 per pair go to d_out."""
        _check(hip_lib().bsw_get_scores_packed_device(self._ctx, ctypes.c_void_p(d_packed), ctypes.byref(desc), w,
                                                      cell_bits, ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))

    def last_stats(self) -> Stats:
        s = Stats()
        _check(hip_lib().bsw_last_stats(self._ctx, ctypes.byref(s)))
        return s

    def sort_order(self, keys: np.ndarray, key_bits: int = 32, use_mask: bool = True) -> np.ndarray:
        """bsw_sort_order_device (test hook, no part of the ABI): the engine's batch-order sort on its own --
        the stable permutation that sorts `keys` by their low key_bits bits; use_mask: digits from the
        varying bits only, as the planned path runs it."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        order = np.empty(len(keys), dtype=np.int32)
        _check(hip_lib().bsw_sort_order_device(self._ctx, _ptr(keys), len(keys), key_bits, int(use_mask), _ptr(order)))
        return order


class Packed(ctypes.Structure):
    """bsw_packed_t: descriptor of a batch in the 2-bit wire form (bsw_pack_batch)"""
    _fields_ = [("n", ctypes.c_int32), ("n_exc_ref", ctypes.c_int32), ("n_exc_qer", ctypes.c_int32),
                ("pad_", ctypes.c_int32), ("ref_bytes", ctypes.c_int64), ("qer_bytes", ctypes.c_int64),
                ("rec_off", ctypes.c_int64), ("ref_off", ctypes.c_int64), ("qer_off", ctypes.c_int64),
                ("exc_off", ctypes.c_int64), ("total_bytes", ctypes.c_int64)]
    FIELDS = ("n", "n_exc_ref", "n_exc_qer", "ref_bytes", "qer_bytes", "rec_off", "ref_off", "qer_off", "exc_off",
              "total_bytes")

    def to_row(self) -> np.ndarray:
        return np.array([getattr(self, f) for f in self.FIELDS], dtype=np.int64)

    @classmethod
    def from_row(cls, row) -> "Packed":
        d = cls()
        for f, v in zip(cls.FIELDS, row):
            setattr(d, f, int(v))
        return d


def pack_batch(pairs: np.ndarray, ref: np.ndarray, qer: np.ndarray, pad_to: int = 0):
    """bsw_pack_batch: (uint8 buffer, Packed) -- the 2-bit wire form of pairs over ref / qer,
    zero-padded to pad_to bytes when that is larger (host-only, no device needed)."""
    assert pairs.dtype == SEQPAIR_DTYPE and pairs.flags.c_contiguous
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    d = Packed()
    L = hip_lib()
    _check(L.bsw_pack_batch(_ptr(pairs), _ptr(ref), _ptr(qer), len(pairs), None, 0, ctypes.byref(d)))
    buf = np.zeros(max(int(d.total_bytes), int(pad_to), 64), dtype=np.uint8)
    _check(L.bsw_pack_batch(_ptr(pairs), _ptr(ref), _ptr(qer), len(pairs), _ptr(buf), len(buf), ctypes.byref(d)))
    return buf, d


def split_by_cells(pairs: np.ndarray, w: int, parts: int) -> np.ndarray:
    """bsw_split_by_cells: parts + 1 cut points of equal static band cells (host-only)."""
    assert pairs.dtype == SEQPAIR_DTYPE and pairs.flags.c_contiguous
    cut = np.zeros(parts + 1, dtype=np.int32)
    _check(hip_lib().bsw_split_by_cells(_ptr(pairs), len(pairs), w, parts, _ptr(cut)))
    return cut


# ---------------------------------------------------------------- .bswb batch files
class BswbHeader(ctypes.Structure):
    """Mirror of bswb_header_t (include/bsw_batch.h), 128 bytes."""
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("header_bytes", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("n_pairs", ctypes.c_int64), ("ref_bytes", ctypes.c_int64),
                ("qer_bytes", ctypes.c_int64), ("checksum", ctypes.c_uint64), ("w", ctypes.c_int32),
                ("cell_bits", ctypes.c_int32), ("params", Params), ("reserved", ctypes.c_uint8 * 20)]


def write_batch(path: str, pairs, ref, qer, w: int, cell_bits: int = 16, params=None,
                has_outputs: bool = True):
    """bswb_write: record a batch (+ outputs) for replay."""
    params = params if params is not None else default_params()
    pairs = np.ascontiguousarray(pairs, dtype=SEQPAIR_DTYPE)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    _check(hip_lib().bswb_write(path.encode(), ctypes.byref(params), w, cell_bits, int(has_outputs),
                                _ptr(pairs), len(pairs), _ptr(ref), len(ref), _ptr(qer), len(qer)))


def read_batch(path: str):
    """bswb_read: (header, pairs, ref, qer); raises BswError on a bad / corrupted file."""
    h = BswbHeader()
    _check(hip_lib().bswb_read_header(path.encode(), ctypes.byref(h)))
    pairs = np.zeros(h.n_pairs, dtype=SEQPAIR_DTYPE)
    ref = np.zeros(max(1, h.ref_bytes), dtype=np.uint8)
    qer = np.zeros(max(1, h.qer_bytes), dtype=np.uint8)
    _check(hip_lib().bswb_read(path.encode(), ctypes.byref(h), _ptr(pairs), _ptr(ref), _ptr(qer)))
    return h, pairs, ref, qer


# ---------------------------------------------------------------- extension pipeline
class ExtOpt(ctypes.Structure):
    """Mirror of bsw_ext_opt_t (include/bsw_ext.h)."""
    _fields_ = [("w", ctypes.c_int32), ("pen_clip5", ctypes.c_int32), ("pen_clip3", ctypes.c_int32),
                ("max_band_try", ctypes.c_int32), ("l_pac", ctypes.c_int64)]


class ExtStats(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int32 * 4), ("kernel_ms", ctypes.c_float), ("build_ms", ctypes.c_float),
                ("engine_ms", ctypes.c_float), ("interp_ms", ctypes.c_float)]


def ext_opt(**kw) -> ExtOpt:
    o = ExtOpt()
    hip_lib().bsw_ext_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def extend_seeds(engine, ref, reads, read_off, read_len, seeds, opt: ExtOpt | None = None):
    """bsw_extend_seeds: one seed per read -> ALNREG_DTYPE regions (local / to-end ends)."""
    opt = opt if opt is not None else ext_opt()
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    out = np.zeros(len(seeds), dtype=ALNREG_DTYPE)
    _check(hip_lib().bsw_extend_seeds(engine._ctx, ctypes.byref(opt), _ptr(ref), len(ref), _ptr(reads),
                                      _ptr(read_off), _ptr(read_len), _ptr(seeds), len(seeds), _ptr(out)))
    return out


def set_reference(engine, ref: np.ndarray):
    """bsw_set_reference: keep ref resident in HBM (for extend_seeds_device)."""
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    _check(hip_lib().bsw_set_reference(engine._ctx, _ptr(ref), len(ref)))


def set_contigs(engine, lens=(), names=()):
    """bsw_set_contigs (include/bsw_contigs.h): the contig table of the resident reference -- lengths and names
    (str or bytes), one each per contig; no contigs removes the table."""
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    if len(lens) != len(names):
        raise ValueError("one name per contig")
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in names]
    arr = (ctypes.c_char_p * max(len(raw), 1))(*raw)
    _check(hip_lib().bsw_set_contigs(engine._ctx, len(lens), _ptr(lens) if len(lens) else None, arr))


def extend_seeds_device(engine, d_reads: int, d_off: int, d_len: int, d_seeds: int, n: int, d_out: int,
                        opt: ExtOpt | None = None, stream: int = 0):
    """bsw_extend_seeds_device on raw device pointers (resident reference required)."""
    opt = opt if opt is not None else ext_opt()
    V = ctypes.c_void_p
    _check(hip_lib().bsw_extend_seeds_device(engine._ctx, ctypes.byref(opt), V(d_reads), V(d_off), V(d_len),
                                             V(d_seeds), n, V(d_out), V(stream or None)))


def extend_seeds_resident(engine, reads, read_off, read_len, seeds, opt: ExtOpt | None = None):
    """Upload reads / seeds, run bsw_extend_seeds_device against the resident reference, download
    the regions (ALNREG_DTYPE)."""
    import hiprt
    bufs = [hiprt.DeviceBuffer.from_array(np.ascontiguousarray(a, dtype=dt)) for a, dt in
            ((reads, np.uint8), (read_off, np.int64), (read_len, np.int32), (seeds, SEED_DTYPE))]
    out = np.zeros(len(seeds), dtype=ALNREG_DTYPE)
    d_out = hiprt.DeviceBuffer(out.nbytes)
    extend_seeds_device(engine, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, len(seeds), d_out.ptr, opt)
    d_out.download(out)
    return out


def ext_last_stats(engine) -> ExtStats:
    s = ExtStats()
    _check(hip_lib().bsw_ext_last_stats(engine._ctx, ctypes.byref(s)))
    return s


# ---------------------------------------------------------------- mate rescue (bsw_mate.h)
class MateStats(ctypes.Structure):
    _fields_ = [("fwd_ms", ctypes.c_float), ("rev_ms", ctypes.c_float), ("n_fwd", ctypes.c_int32),
                ("n_rev", ctypes.c_int32), ("cells_fwd", ctypes.c_int64)]


def ksw_align2(engine, pairs: np.ndarray, ref: np.ndarray, qer: np.ndarray) -> np.ndarray:
    """bsw_ksw_align2: per SeqPair (len1 = target, len2 = query, h0 = xtra) upstream
    ksw_align2's kswr_t -> KSWR_DTYPE array."""
    assert pairs.dtype == SEQPAIR_DTYPE and pairs.flags.c_contiguous
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    out = np.zeros(len(pairs), dtype=KSWR_DTYPE)
    _check(hip_lib().bsw_ksw_align2(engine._ctx, _ptr(pairs), _ptr(ref), _ptr(qer), len(pairs), _ptr(out)))
    return out


def ksw_align2_device(engine, d_pairs: int, d_ref: int, d_qer: int, n: int, d_aln: int, stream: int = 0):
    _check(hip_lib().bsw_ksw_align2_device(engine._ctx, ctypes.c_void_p(d_pairs), ctypes.c_void_p(d_ref),
                                           ctypes.c_void_p(d_qer), n, ctypes.c_void_p(d_aln),
                                           ctypes.c_void_p(stream or None)))


def mate_last_stats(engine) -> MateStats:
    s = MateStats()
    _check(hip_lib().bsw_mate_last_stats(engine._ctx, ctypes.byref(s)))
    return s


class GlobalStats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_float), ("n_jobs", ctypes.c_int32), ("n_lane", ctypes.c_int32),
                ("n_wide", ctypes.c_int32), ("n_launches", ctypes.c_int32), ("cells", ctypes.c_int64),
                ("z_bytes", ctypes.c_int64), ("n_tb_retry", ctypes.c_int32), ("pad_", ctypes.c_int32)]


def ksw_global2(engine, pairs: np.ndarray, ref: np.ndarray, qer: np.ndarray, stride: int = 64):
    """bsw_ksw_global2 (include/bsw_global.h): per SeqPair (len1 = target, len2 = query, h0 = w)
    upstream ksw_global2 -> (score, cigar[n, stride] uint32 or None, n_cigar); scores are also
    written into pairs['score']."""
    assert pairs.dtype == SEQPAIR_DTYPE and pairs.flags.c_contiguous
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    n = len(pairs)
    cig = np.zeros((n, stride), dtype=np.uint32) if stride > 0 else None
    ncig = np.zeros(n, dtype=np.int32)
    _check(hip_lib().bsw_ksw_global2(engine._ctx, _ptr(pairs), _ptr(ref), _ptr(qer), n,
                                     _ptr(cig) if cig is not None else None, stride, _ptr(ncig)))
    return pairs["score"].copy(), cig, ncig


def ksw_global2_device(engine, d_pairs: int, d_ref: int, d_qer: int, n: int, d_cigar: int, stride: int,
                       d_ncig: int, stream: int = 0):
    _check(hip_lib().bsw_ksw_global2_device(engine._ctx, ctypes.c_void_p(d_pairs), ctypes.c_void_p(d_ref),
                                            ctypes.c_void_p(d_qer), n, ctypes.c_void_p(d_cigar or None),
                                            stride, ctypes.c_void_p(d_ncig or None),
                                            ctypes.c_void_p(stream or None)))


def global_last_stats(engine) -> GlobalStats:
    s = GlobalStats()
    _check(hip_lib().bsw_global_last_stats(engine._ctx, ctypes.byref(s)))
    return s


# ---------------------------------------------------------------- synthetic batches
class SynthCfg(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("tlen", ctypes.c_int32), ("qlen", ctypes.c_int32),
                ("h0_lo", ctypes.c_int32), ("h0_hi", ctypes.c_int32),
                ("p_sub", ctypes.c_double), ("p_indel", ctypes.c_double),
                ("p_unrelated", ctypes.c_double), ("p_n", ctypes.c_double)]


_synth = None


def synth_lib():
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_LIB):
            raise BswError(f"{SYNTH_LIB} not built: run `make synth`")
        L = ctypes.CDLL(SYNTH_LIB)
        L.bsw_synth_default.argtypes = [ctypes.c_void_p]
        L.bsw_synth_batch.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.bsw_synth_reference.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p]
        L.bsw_reads_default.argtypes = [ctypes.c_void_p]
        L.bsw_synth_reads.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.bsw_synth_reads.restype = ctypes.c_int32
        L.bsw_synth_pe_seeds.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.bsw_synth_pe_seeds.restype = ctypes.c_int32
        L.bsw_mates_default.argtypes = [ctypes.c_void_p]
        L.bsw_synth_mates.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.bsw_synth_mates.restype = ctypes.c_int32
        L.bsw_globals_default.argtypes = [ctypes.c_void_p]
        L.bsw_synth_globals.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.bsw_synth_globals.restype = ctypes.c_int32
        _synth = L
    return _synth


def synth_cfg(**kw) -> SynthCfg:
    c = SynthCfg()
    synth_lib().bsw_synth_default(ctypes.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def synth_batch(n: int, pair_base: int = 0, cfg: SynthCfg | None = None):
    """C2 workload batch: (pairs, ref, qer) numpy arrays in the upstream layout."""
    cfg = cfg if cfg is not None else synth_cfg()
    pairs = np.zeros(n, dtype=SEQPAIR_DTYPE)
    ref = np.zeros(max(1, n * cfg.tlen), dtype=np.uint8)
    qer = np.zeros(max(1, n * cfg.qlen), dtype=np.uint8)
    synth_lib().bsw_synth_batch(ctypes.byref(cfg), pair_base, n, _ptr(pairs), _ptr(ref),
                                _ptr(qer))
    return pairs, ref, qer


class ReadsCfg(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("read_len", ctypes.c_int32), ("min_seed", ctypes.c_int32),
                ("p_sub", ctypes.c_double), ("p_indel", ctypes.c_double), ("p_unrelated", ctypes.c_double)]


def reads_cfg(**kw) -> ReadsCfg:
    c = ReadsCfg()
    synth_lib().bsw_reads_default(ctypes.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def synth_reference(length: int, seed: int = 7, p_n: float = 0.0005) -> np.ndarray:
    """Random reference (codes 0..3, N = 4 at rate p_n), reproducible per seed."""
    ref = np.empty(length, dtype=np.uint8)
    synth_lib().bsw_synth_reference(seed, length, p_n, _ptr(ref))
    return ref


def synth_reads(ref: np.ndarray, n: int, read_base: int = 0, cfg: ReadsCfg | None = None):
    """Reads sampled from ref with one exact seed each: (reads, read_off, read_len, seeds, origin)."""
    cfg = cfg if cfg is not None else reads_cfg()
    L = cfg.read_len
    reads = np.zeros(max(1, n * L), dtype=np.uint8)
    seeds = np.zeros(n, dtype=SEED_DTYPE)
    origin = np.zeros(n, dtype=np.int64)
    r = synth_lib().bsw_synth_reads(ctypes.byref(cfg), _ptr(ref), len(ref), read_base, n, _ptr(reads),
                                    _ptr(seeds), _ptr(origin))
    if r < 0:
        raise BswError("bsw_synth_reads: reference too short for the read length")
    read_off = np.arange(n, dtype=np.int64) * L
    read_len = np.full(n, L, dtype=np.int32)
    return reads, read_off, read_len, seeds, origin


def synth_pe_seeds(ref: np.ndarray, n_pairs: int, pair_base: int = 0, cfg: ReadsCfg | None = None,
                   ins=(400, 600), p_spurious: float = 0.1):
    """Paired-end reads with several seeds each (bsw_synth_pe_seeds): (reads, read_off, read_len,
    seeds, seed_read, seed_chain); read_off / read_len are PER READ (2 n_pairs reads; reads 2k /
    2k+1 are the mates of fragment k), seed_read / seed_chain map each seed to its read and chain
    (bsw_chain2aln's input layout; for bsw_extend_seeds index read_off by seed_read)."""
    cfg = cfg if cfg is not None else reads_cfg()
    L = cfg.read_len
    n_reads = 2 * n_pairs
    reads = np.zeros(max(1, n_reads * L), dtype=np.uint8)
    seeds = np.zeros(max(1, n_reads * 9), dtype=SEED_DTYPE)
    seed_read = np.zeros(max(1, n_reads * 9), dtype=np.int32)
    seed_chain = np.zeros(max(1, n_reads * 9), dtype=np.int32)
    ns = synth_lib().bsw_synth_pe_seeds(ctypes.byref(cfg), _ptr(ref), len(ref), pair_base, n_pairs, ins[0], ins[1],
                                        ctypes.c_double(p_spurious), _ptr(reads), _ptr(seeds), _ptr(seed_read),
                                        _ptr(seed_chain))
    if ns < 0:
        raise BswError("bsw_synth_pe_seeds: reference too short")
    read_off = np.arange(n_reads, dtype=np.int64) * L
    read_len = np.full(n_reads, L, dtype=np.int32)
    return reads, read_off, read_len, seeds[:ns].copy(), seed_read[:ns].copy(), seed_chain[:ns].copy()


class ChainStats(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_int32), ("n_extended", ctypes.c_int32), ("n_skipped", ctypes.c_int32),
                ("n_pairs", ctypes.c_int32 * 4), ("kernel_ms", ctypes.c_float), ("ext_ms", ctypes.c_float),
                ("check_ms", ctypes.c_float), ("prep_ms", ctypes.c_float)]


def chain2aln(engine, ref, reads, read_off, read_len, seeds, seed_read, seed_chain, opt: ExtOpt | None = None):
    """bsw_chain2aln: (regions per seed, extended flags)."""
    opt = opt if opt is not None else ext_opt()
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    seed_read = np.ascontiguousarray(seed_read, dtype=np.int32)
    seed_chain = np.ascontiguousarray(seed_chain, dtype=np.int32)
    out = np.zeros(len(seeds), dtype=ALNREG_DTYPE)
    ext = np.zeros(len(seeds), dtype=np.int32)
    _check(hip_lib().bsw_chain2aln(engine._ctx, ctypes.byref(opt), _ptr(ref), len(ref), _ptr(reads), _ptr(read_off),
                                   _ptr(read_len), len(read_len), _ptr(seeds), _ptr(seed_read), _ptr(seed_chain),
                                   len(seeds), _ptr(out), _ptr(ext)))
    return out, ext


def chain2aln_device(engine, d_reads: int, read_off, read_len, seeds, seed_read, seed_chain,
                     opt: ExtOpt | None = None, out=None, ext=None):
    """bsw_chain2aln_device: reads resident at d_reads (device pointer), reference resident;
    `out` / `ext` may be preallocated (ALNREG_DTYPE / int32, len(seeds))."""
    opt = opt if opt is not None else ext_opt()
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    seed_read = np.ascontiguousarray(seed_read, dtype=np.int32)
    seed_chain = np.ascontiguousarray(seed_chain, dtype=np.int32)
    out = np.zeros(len(seeds), dtype=ALNREG_DTYPE) if out is None else out
    ext = np.zeros(len(seeds), dtype=np.int32) if ext is None else ext
    assert out.dtype == ALNREG_DTYPE and len(out) == len(seeds) and ext.dtype == np.int32 and len(ext) == len(seeds)
    _check(hip_lib().bsw_chain2aln_device(engine._ctx, ctypes.byref(opt), ctypes.c_void_p(d_reads), _ptr(read_off),
                                          _ptr(read_len), len(read_len), _ptr(seeds), _ptr(seed_read),
                                          _ptr(seed_chain), len(seeds), _ptr(out), _ptr(ext)))
    return out, ext


def chain2aln_resident(engine, d_reads: int, d_off: int, d_len: int, n_reads: int, d_seeds: int, d_sr: int,
                       d_sc: int, n_seeds: int, d_out: int, d_ext: int, opt: ExtOpt | None = None):
    """bsw_chain2aln_resident: every array a device pointer (regions / flags into d_out / d_ext)."""
    opt = opt if opt is not None else ext_opt()
    V = ctypes.c_void_p
    _check(hip_lib().bsw_chain2aln_resident(engine._ctx, ctypes.byref(opt), V(d_reads), V(d_off), V(d_len), n_reads,
                                            V(d_seeds), V(d_sr), V(d_sc), n_seeds, V(d_out), V(d_ext)))


def chain_last_stats(engine) -> ChainStats:
    st = ChainStats()
    _check(hip_lib().bsw_chain_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- final alignments (bsw_aln.h)
class AlnStats(ctypes.Structure):
    _fields_ = [("n_regs", ctypes.c_int32), ("n_rejected", ctypes.c_int32), ("n_gapfree", ctypes.c_int32),
                ("n_dp", ctypes.c_int32 * 3), ("dp_ms", ctypes.c_float), ("helper_ms", ctypes.c_float)]


def reg2aln(engine, reads, read_off, read_len, regs, reg_read, opt: ExtOpt | None = None, cigar_stride: int = 16,
            md_stride: int = 64):
    """bsw_reg2aln (host arrays, resident reference required): regions (ALNREG_DTYPE) of reads
    reg_read[k] -> (aln ALN_DTYPE, cigar [n, cigar_stride] uint32, md [n, md_stride] uint8 or None
    when md_stride == 0)."""
    opt = opt if opt is not None else ext_opt()
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    regs = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
    reg_read = np.ascontiguousarray(reg_read, dtype=np.int32)
    n = len(regs)
    aln = np.zeros(n, dtype=ALN_DTYPE)
    cig = np.zeros((n, cigar_stride), dtype=np.uint32)
    md = np.zeros((n, md_stride), dtype=np.uint8) if md_stride > 0 else None
    _check(hip_lib().bsw_reg2aln(engine._ctx, ctypes.byref(opt), _ptr(reads), _ptr(read_off), _ptr(read_len),
                                 len(read_len), _ptr(regs), _ptr(reg_read), n, _ptr(aln), _ptr(cig), cigar_stride,
                                 _ptr(md) if md is not None else None, md_stride))
    return aln, cig, md


def reg2aln_resident(engine, d_reads: int, d_off: int, d_len: int, n_reads: int, d_regs: int, d_reg_read: int,
                     n_regs: int, d_aln: int, d_cigar: int, cigar_stride: int, d_md: int, md_stride: int,
                     opt: ExtOpt | None = None, stream: int = 0):
    """bsw_reg2aln_resident: every array a device pointer (d_regs / d_reg_read as
    bsw_chain2aln_resident leaves them in d_out / d_seed_read)."""
    opt = opt if opt is not None else ext_opt()
    V = ctypes.c_void_p
    _check(hip_lib().bsw_reg2aln_resident(engine._ctx, ctypes.byref(opt), V(d_reads), V(d_off), V(d_len), n_reads,
                                          V(d_regs), V(d_reg_read), n_regs, V(d_aln), V(d_cigar), cigar_stride,
                                          V(d_md or None), md_stride, V(stream or None)))


def aln_last_stats(engine) -> AlnStats:
    st = AlnStats()
    _check(hip_lib().bsw_aln_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- region selection (bsw_sel.h)
class SelOpt(ctypes.Structure):
    """Mirror of bsw_sel_opt_t (include/bsw_sel.h)."""
    _fields_ = [("w", ctypes.c_int32), ("max_chain_gap", ctypes.c_int32), ("l_pac", ctypes.c_int64),
                ("mask_level_redun", ctypes.c_float), ("mask_level", ctypes.c_float),
                ("min_seed_len", ctypes.c_int32), ("b", ctypes.c_int32), ("mapQ_coef_len", ctypes.c_int32),
                ("mapQ_coef_fac", ctypes.c_int32), ("patch", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("id0", ctypes.c_int64)]


class SelStats(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int32), ("n_regs_in", ctypes.c_int32), ("n_redundant", ctypes.c_int32),
                ("n_identical", ctypes.c_int32), ("n_patch_tried", ctypes.c_int32), ("n_patch_ok", ctypes.c_int32),
                ("n_patch_ratio", ctypes.c_int32), ("n_dp", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("n_sel", ctypes.c_int32), ("dp_ms", ctypes.c_float), ("helper_ms", ctypes.c_float)]


def sel_opt(**kw) -> SelOpt:
    o = SelOpt()
    hip_lib().bsw_sel_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def regs_select(engine, reads, read_off, read_len, seeds, seed_read, seed_chain, regs, extended,
                opt: SelOpt | None = None, csub=None, frac_rep=None, sel_cap: int | None = None):
    """bsw_regs_select (host arrays, resident reference required): the regions bsw_chain2aln* left
    -> (sel_regs ALNREG_DTYPE, sel_read int32, sel_info SELINFO_DTYPE, read_first int32 [n_reads + 1]).
    A sel_cap below the number kept raises BswError with .needed set."""
    opt = opt if opt is not None else sel_opt()
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    seed_read = np.ascontiguousarray(seed_read, dtype=np.int32)
    seed_chain = np.ascontiguousarray(seed_chain, dtype=np.int32)
    regs = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
    extended = np.ascontiguousarray(extended, dtype=np.int32)
    csub = None if csub is None else np.ascontiguousarray(csub, dtype=np.int32)
    frac_rep = None if frac_rep is None else np.ascontiguousarray(frac_rep, dtype=np.float32)
    n = len(seeds)
    assert len(seed_read) == len(seed_chain) == len(regs) == len(extended) == n
    assert (csub is None or len(csub) == n) and (frac_rep is None or len(frac_rep) == len(read_len))
    cap = n if sel_cap is None else sel_cap
    sel_regs = np.zeros(max(cap, 1), dtype=ALNREG_DTYPE)
    sel_read = np.zeros(max(cap, 1), dtype=np.int32)
    sel_info = np.zeros(max(cap, 1), dtype=SELINFO_DTYPE)
    first = np.zeros(len(read_len) + 1, dtype=np.int32)
    n_sel = ctypes.c_int32(-1)
    rc = hip_lib().bsw_regs_select(engine._ctx, ctypes.byref(opt), _ptr(reads), _ptr(read_off), _ptr(read_len),
                                   len(read_len), _ptr(seeds), _ptr(seed_read), _ptr(seed_chain), _ptr(regs),
                                   _ptr(extended), n, _ptr(csub) if csub is not None else None,
                                   _ptr(frac_rep) if frac_rep is not None else None, _ptr(sel_regs), _ptr(sel_read),
                                   _ptr(sel_info), _ptr(first), cap, ctypes.byref(n_sel))
    if rc != 0:
        try:
            _check(rc)
        except BswError as e:
            e.needed = n_sel.value
            raise
    k = n_sel.value
    return sel_regs[:k], sel_read[:k], sel_info[:k], first


def regs_select_resident(engine, d_reads: int, d_off: int, d_len: int, n_reads: int, d_seeds: int, d_sr: int,
                         d_sc: int, d_regs: int, d_ext: int, n_seeds: int, d_sel_regs: int, d_sel_read: int,
                         d_sel_info: int, d_read_first: int, sel_cap: int, opt: SelOpt | None = None,
                         d_csub: int = 0, d_frac_rep: int = 0, stream: int = 0) -> int:
    """bsw_regs_select_resident: every array a device pointer (the inputs as bsw_chain2aln_resident
    takes and leaves them; d_sel_regs / d_sel_read feed bsw_reg2aln_resident).  Returns n_sel."""
    opt = opt if opt is not None else sel_opt()
    V = ctypes.c_void_p
    n_sel = ctypes.c_int32(-1)
    rc = hip_lib().bsw_regs_select_resident(engine._ctx, ctypes.byref(opt), V(d_reads), V(d_off), V(d_len), n_reads,
                                            V(d_seeds), V(d_sr), V(d_sc), V(d_regs), V(d_ext), n_seeds,
                                            V(d_csub or None), V(d_frac_rep or None), V(d_sel_regs), V(d_sel_read),
                                            V(d_sel_info), V(d_read_first), sel_cap, ctypes.byref(n_sel),
                                            V(stream or None))
    if rc != 0:
        try:
            _check(rc)
        except BswError as e:
            e.needed = n_sel.value
            raise
    return n_sel.value


def sel_last_stats(engine) -> SelStats:
    st = SelStats()
    _check(hip_lib().bsw_sel_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- paired-end stage (bsw_pe.h)
class PeOpt(ctypes.Structure):
    """Mirror of bsw_pe_opt_t (include/bsw_pe.h)."""
    _fields_ = [("l_pac", ctypes.c_int64), ("id0", ctypes.c_int64), ("max_ins", ctypes.c_int32),
                ("min_seed_len", ctypes.c_int32), ("b", ctypes.c_int32), ("T", ctypes.c_int32),
                ("pen_unpaired", ctypes.c_int32), ("mapQ_coef_len", ctypes.c_int32), ("mapQ_coef_fac", ctypes.c_int32),
                ("mask_level", ctypes.c_float)]


class PeStats(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int32), ("n_cand", ctypes.c_int32 * 4), ("n_pairing_tried", ctypes.c_int32),
                ("n_paired", ctypes.c_int32), ("n_multi", ctypes.c_int32), ("n_unpaired_preferred", ctypes.c_int32),
                ("n_proper", ctypes.c_int32), ("n_u", ctypes.c_int64), ("kernel_ms", ctypes.c_float),
                ("reserved", ctypes.c_int32)]


def pe_opt(**kw) -> PeOpt:
    o = PeOpt()
    hip_lib().bsw_pe_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _pe_host(sel_regs, sel_info, read_first):
    sel_regs = np.ascontiguousarray(sel_regs, dtype=ALNREG_DTYPE)
    sel_info = np.ascontiguousarray(sel_info, dtype=SELINFO_DTYPE)
    read_first = np.ascontiguousarray(read_first, dtype=np.int32)
    assert len(read_first) >= 1 and len(sel_regs) == len(sel_info)
    return sel_regs, sel_info, read_first


def pe_stat(engine, sel_regs, sel_info, read_first, opt: PeOpt) -> np.ndarray:
    """bsw_pe_stat (host arrays as bsw_regs_select returns them) -> pes PESTAT_DTYPE [4]."""
    sel_regs, sel_info, read_first = _pe_host(sel_regs, sel_info, read_first)
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    _check(hip_lib().bsw_pe_stat(engine._ctx, ctypes.byref(opt), _ptr(sel_regs), _ptr(sel_info), _ptr(read_first),
                                 len(read_first) - 1, _ptr(pes)))
    return pes


def pe_stat_resident(engine, d_sel_regs: int, d_sel_info: int, d_read_first: int, n_reads: int, n_regs: int,
                     opt: PeOpt, stream: int = 0) -> np.ndarray:
    """bsw_pe_stat_resident: the arrays bsw_regs_select_resident left, as device pointers."""
    V = ctypes.c_void_p
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    _check(hip_lib().bsw_pe_stat_resident(engine._ctx, ctypes.byref(opt), V(d_sel_regs or None), V(d_sel_info or None),
                                          V(d_read_first), n_reads, n_regs, _ptr(pes), V(stream or None)))
    return pes


def pe_pair(engine, pes, sel_regs, sel_info, read_first, opt: PeOpt):
    """bsw_pe_pair on copies of the host arrays -> (sel_regs, sel_info, pairs PAIR_DTYPE [n_reads / 2])."""
    sel_regs, sel_info, read_first = _pe_host(sel_regs, sel_info, read_first)
    sel_regs, sel_info = sel_regs.copy(), sel_info.copy()
    pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
    assert len(pes) == 4
    n_reads = len(read_first) - 1
    pairs = np.zeros(max(n_reads // 2, 1), dtype=PAIR_DTYPE)
    _check(hip_lib().bsw_pe_pair(engine._ctx, ctypes.byref(opt), _ptr(pes), _ptr(sel_regs), _ptr(sel_info),
                                 _ptr(read_first), n_reads, _ptr(pairs)))
    return sel_regs, sel_info, pairs[:n_reads // 2]


def pe_pair_resident(engine, pes, d_sel_regs: int, d_sel_info: int, d_read_first: int, n_reads: int, n_regs: int,
                     d_pairs: int, opt: PeOpt, stream: int = 0):
    """bsw_pe_pair_resident: d_sel_regs / d_sel_info are updated in place, d_pairs written."""
    V = ctypes.c_void_p
    pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
    assert len(pes) == 4
    _check(hip_lib().bsw_pe_pair_resident(engine._ctx, ctypes.byref(opt), _ptr(pes), V(d_sel_regs or None),
                                          V(d_sel_info or None), V(d_read_first), n_reads, n_regs, V(d_pairs or None),
                                          V(stream or None)))


def pe_last_stats(engine) -> PeStats:
    st = PeStats()
    _check(hip_lib().bsw_pe_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- mate rescue stage (bsw_matesw.h)
class MateswOpt(ctypes.Structure):
    """Mirror of bsw_matesw_opt_t (include/bsw_matesw.h)."""
    _fields_ = [("l_pac", ctypes.c_int64), ("max_matesw", ctypes.c_int32), ("pen_unpaired", ctypes.c_int32),
                ("min_seed_len", ctypes.c_int32), ("max_chain_gap", ctypes.c_int32),
                ("mask_level_redun", ctypes.c_float), ("reserved", ctypes.c_int32)]


class MateswStats(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int32), ("n_calls", ctypes.c_int32), ("n_calls_all_skipped", ctypes.c_int32),
                ("n_jobs", ctypes.c_int32), ("n_jobs_u8", ctypes.c_int32), ("n_short_window", ctypes.c_int32),
                ("n_pushed", ctypes.c_int32), ("n_redundant", ctypes.c_int32), ("n_identical", ctypes.c_int32),
                ("n_lists_changed", ctypes.c_int32), ("rounds", ctypes.c_int32), ("n_out", ctypes.c_int32),
                ("sw_ms", ctypes.c_float), ("helper_ms", ctypes.c_float)]


def matesw_opt(**kw) -> MateswOpt:
    o = MateswOpt()
    hip_lib().bsw_matesw_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _raise_needed(rc, n_out):
    try:
        _check(rc)
    except BswError as e:
        e.needed = n_out.value
        raise


def matesw(engine, pes, reads, read_off, read_len, sel_regs, sel_info, read_first, opt: MateswOpt,
           out_cap: int | None = None):
    """bsw_matesw (host arrays, resident reference required): the lists bsw_regs_select left and the
    pes of bsw_pe_stat -> (regs ALNREG_DTYPE, reg_read int32, info SELINFO_DTYPE, first int32
    [n_reads + 1]) for bsw_pe_pair / bsw_reg2aln.  An out_cap below the number needed raises BswError
    with .needed set (and .first, the offsets, which are still written)."""
    sel_regs, sel_info, read_first = _pe_host(sel_regs, sel_info, read_first)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
    n_reads = len(read_first) - 1
    assert len(pes) == 4 and len(read_off) == len(read_len) == n_reads
    cap = len(sel_regs) + 4 * opt.max_matesw * n_reads if out_cap is None else out_cap
    regs = np.zeros(max(cap, 1), dtype=ALNREG_DTYPE)
    rd = np.zeros(max(cap, 1), dtype=np.int32)
    info = np.zeros(max(cap, 1), dtype=SELINFO_DTYPE)
    first = np.zeros(n_reads + 1, dtype=np.int32)
    n_out = ctypes.c_int32(-1)
    rc = hip_lib().bsw_matesw(engine._ctx, ctypes.byref(opt), _ptr(pes), _ptr(reads), _ptr(read_off), _ptr(read_len),
                              n_reads, _ptr(sel_regs), _ptr(sel_info), _ptr(read_first), _ptr(regs), _ptr(rd),
                              _ptr(info), _ptr(first), cap, ctypes.byref(n_out))
    if rc != 0:
        try:
            _raise_needed(rc, n_out)
        except BswError as e:
            e.first = first
            raise
    k = n_out.value
    return regs[:k], rd[:k], info[:k], first


def matesw_resident(engine, pes, d_reads: int, d_off: int, d_len: int, n_reads: int, d_sel_regs: int, d_sel_info: int,
                    d_read_first: int, n_regs: int, d_out_regs: int, d_out_read: int, d_out_info: int,
                    d_out_first: int, out_cap: int, opt: MateswOpt, stream: int = 0) -> int:
    """bsw_matesw_resident: every array a device pointer (the inputs as bsw_regs_select_resident took
    and left them; the outputs feed bsw_pe_pair_resident and bsw_reg2aln_resident).  Returns n_out."""
    V = ctypes.c_void_p
    pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
    assert len(pes) == 4
    n_out = ctypes.c_int32(-1)
    rc = hip_lib().bsw_matesw_resident(engine._ctx, ctypes.byref(opt), _ptr(pes), V(d_reads or None), V(d_off or None),
                                       V(d_len or None), n_reads, V(d_sel_regs or None), V(d_sel_info or None),
                                       V(d_read_first), n_regs, V(d_out_regs or None), V(d_out_read or None),
                                       V(d_out_info or None), V(d_out_first), out_cap, ctypes.byref(n_out),
                                       V(stream or None))
    if rc != 0:
        _raise_needed(rc, n_out)
    return n_out.value


def matesw_last_stats(engine) -> MateswStats:
    st = MateswStats()
    _check(hip_lib().bsw_matesw_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- SAM records (bsw_rec.h)
class RecOpt(ctypes.Structure):
    """Mirror of bsw_rec_opt_t (include/bsw_rec.h)."""
    _fields_ = [("l_pac", ctypes.c_int64), ("w", ctypes.c_int32), ("T", ctypes.c_int32), ("max_XA_hits", ctypes.c_int32),
                ("XA_drop_ratio", ctypes.c_float), ("mask_level", ctypes.c_float), ("flags", ctypes.c_int32),
                ("rname", ctypes.c_char * 64)]


class RecStats(ctypes.Structure):
    _fields_ = [("n_rec", ctypes.c_int32), ("n_unmapped", ctypes.c_int32), ("n_supp", ctypes.c_int32),
                ("n_xa", ctypes.c_int32), ("n_aln", ctypes.c_int32), ("n_overflow", ctypes.c_int32),
                ("n_bytes", ctypes.c_int64), ("aln_ms", ctypes.c_float), ("helper_ms", ctypes.c_float),
                ("text_ms", ctypes.c_float), ("reserved", ctypes.c_int32)]


def rec_opt(**kw) -> RecOpt:
    o = RecOpt()
    hip_lib().bsw_rec_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v.encode() if isinstance(v, str) else v)
    return o


def _raise_rec(rc, n_rec, n_aln, rec_first=None):
    try:
        _check(rc)
    except BswError as e:
        e.needed = (n_rec.value, n_aln.value)
        e.rec_first = rec_first
        raise


def records(engine, reads, read_off, read_len, sel_regs, sel_info, read_first, pairs, opt: RecOpt, cigar_stride: int = 16,
            md_stride: int = 64, rec_cap: int | None = None, aln_cap: int | None = None):
    """bsw_records (host arrays, resident reference required): the lists bsw_pe_pair (with its pairs) or
    bsw_regs_select (pairs=None) left -> (recs REC_DTYPE, rec_first int32 [n_reads + 1], aln ALN_DTYPE, aln_reg
    int32, cigar [n_aln, cigar_stride] uint32, md [n_aln, md_stride] uint8).  A capacity below what is needed
    raises BswError with .needed = (n_rec, n_aln) and .rec_first set."""
    sel_regs, sel_info, read_first = _pe_host(sel_regs, sel_info, read_first)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    n_reads = len(read_first) - 1
    assert len(read_off) == len(read_len) == n_reads and (pairs is None or len(pairs) == n_reads // 2)
    rc_ = n_reads + len(sel_regs) if rec_cap is None else rec_cap
    ac = len(sel_regs) if aln_cap is None else aln_cap
    recs = np.zeros(max(rc_, 1), dtype=REC_DTYPE)
    first = np.zeros(n_reads + 1, dtype=np.int32)
    aln = np.zeros(max(ac, 1), dtype=ALN_DTYPE)
    aln_reg = np.zeros(max(ac, 1), dtype=np.int32)
    cig = np.zeros((max(ac, 1), cigar_stride), dtype=np.uint32)
    md = np.zeros((max(ac, 1), max(md_stride, 1)), dtype=np.uint8)
    n_rec, n_aln = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = hip_lib().bsw_records(engine._ctx, ctypes.byref(opt), _ptr(reads), _ptr(read_off), _ptr(read_len), n_reads,
                               _ptr(sel_regs), _ptr(sel_info), _ptr(read_first), _ptr(pairs) if pairs is not None else None,
                               _ptr(recs), _ptr(first), rc_, _ptr(aln), _ptr(aln_reg), _ptr(cig), cigar_stride, _ptr(md),
                               md_stride, ac, ctypes.byref(n_rec), ctypes.byref(n_aln))
    if rc != 0:
        _raise_rec(rc, n_rec, n_aln, first)
    k, m = n_rec.value, n_aln.value
    return recs[:k], first, aln[:m], aln_reg[:m], cig[:m], md[:m]


def records_resident(engine, d_reads: int, d_off: int, d_len: int, n_reads: int, d_sel_regs: int, d_sel_info: int,
                     d_read_first: int, n_regs: int, d_pairs: int, d_recs: int, d_rec_first: int, rec_cap: int,
                     d_aln: int, d_aln_reg: int, d_cigar: int, cigar_stride: int, d_md: int, md_stride: int,
                     aln_cap: int, opt: RecOpt, stream: int = 0):
    """bsw_records_resident: every array a device pointer (the inputs as bsw_pe_pair_resident or
    bsw_regs_select_resident left them; d_pairs = 0 for single-end).  Returns (n_rec, n_aln)."""
    V = ctypes.c_void_p
    n_rec, n_aln = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = hip_lib().bsw_records_resident(engine._ctx, ctypes.byref(opt), V(d_reads or None), V(d_off or None),
                                        V(d_len or None), n_reads, V(d_sel_regs or None), V(d_sel_info or None),
                                        V(d_read_first), n_regs, V(d_pairs or None), V(d_recs or None), V(d_rec_first),
                                        rec_cap, V(d_aln or None), V(d_aln_reg or None), V(d_cigar or None), cigar_stride,
                                        V(d_md or None), md_stride, aln_cap, ctypes.byref(n_rec), ctypes.byref(n_aln),
                                        V(stream or None))
    if rc != 0:
        _raise_rec(rc, n_rec, n_aln)
    return n_rec.value, n_aln.value


def _names_host(names):
    """list of bytes -> (bytes uint8, offsets int64 [n + 1])"""
    off = np.zeros(len(names) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in names])
    flat = np.frombuffer(b"".join(names), dtype=np.uint8).copy() if len(names) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat if len(flat) else np.zeros(1, np.uint8)), off


def sam_text(engine, recs, rec_first, aln, cigar, md, reads, read_off, read_len, names, quals, opt: RecOpt,
             paired: bool, text_cap: int | None = None):
    """bsw_sam_text (host arrays): bsw_records' outputs, the reads, names (a list of bytes, one per read or per
    pair) and quals (uint8 parallel to reads, or None) -> (text bytes, text_off int64 [n_rec + 1]).  A text_cap
    below what is needed raises BswError with .needed set."""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    rec_first = np.ascontiguousarray(rec_first, dtype=np.int32)
    aln = np.ascontiguousarray(aln, dtype=ALN_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    md = np.ascontiguousarray(md, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    quals = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
    nm, nm_off = _names_host(names)
    n_reads = len(read_len)
    assert len(names) == (n_reads // 2 if paired else n_reads) and (quals is None or len(quals) == len(reads))
    cs = cigar.shape[1] if cigar.ndim == 2 else 1
    ms = md.shape[1] if md.ndim == 2 else 1
    if text_cap is None:        # a bound on any line: the name, the fixed fields, SEQ + QUAL, MD, and 12 bytes per CIGAR op printed
        per = 256 + 160 + 2 * int(read_len.max(initial=0)) + ms + 12 * cs * 16
        text_cap = per * max(len(recs), 1)
    text = np.zeros(max(text_cap, 1), dtype=np.uint8)
    text_off = np.zeros(len(recs) + 1, dtype=np.int64)
    n_bytes = ctypes.c_int64(-1)
    rc = hip_lib().bsw_sam_text(engine._ctx, ctypes.byref(opt), _ptr(recs), _ptr(rec_first), len(recs), _ptr(aln),
                                _ptr(cigar), cs, _ptr(md), ms, len(aln), _ptr(reads), _ptr(read_off), _ptr(read_len),
                                n_reads, _ptr(nm), _ptr(nm_off), _ptr(quals) if quals is not None else None, int(paired),
                                _ptr(text), _ptr(text_off), text_cap, ctypes.byref(n_bytes))
    if rc != 0:
        try:
            _raise_needed(rc, n_bytes)
        except BswError as e:
            e.text_off = text_off
            raise
    return text[:n_bytes.value].tobytes(), text_off


def sam_text_resident(engine, d_recs: int, d_rec_first: int, n_rec: int, d_aln: int, d_cigar: int, cigar_stride: int,
                      d_md: int, md_stride: int, n_aln: int, d_reads: int, d_off: int, d_len: int, n_reads: int,
                      d_names: int, d_name_off: int, d_quals: int, paired: bool, d_text: int, d_text_off: int,
                      text_cap: int, opt: RecOpt, stream: int = 0) -> int:
    """bsw_sam_text_resident: every array a device pointer.  Returns n_bytes."""
    V = ctypes.c_void_p
    n_bytes = ctypes.c_int64(-1)
    rc = hip_lib().bsw_sam_text_resident(engine._ctx, ctypes.byref(opt), V(d_recs or None), V(d_rec_first or None), n_rec,
                                         V(d_aln or None), V(d_cigar or None), cigar_stride, V(d_md or None), md_stride,
                                         n_aln, V(d_reads or None), V(d_off or None), V(d_len or None), n_reads,
                                         V(d_names or None), V(d_name_off), V(d_quals or None), int(paired),
                                         V(d_text or None), V(d_text_off), text_cap, ctypes.byref(n_bytes),
                                         V(stream or None))
    if rc != 0:
        _raise_needed(rc, n_bytes)
    return n_bytes.value


def rec_last_stats(engine) -> RecStats:
    st = RecStats()
    _check(hip_lib().bsw_rec_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- BAM records (bsw_bam.h)
class BamStats(ctypes.Structure):
    _fields_ = [("n_rec", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_bytes", ctypes.c_int64),
                ("len_ms", ctypes.c_float), ("write_ms", ctypes.c_float)]


def bam_records(engine, recs, rec_first, aln, cigar, md, reads, read_off, read_len, names, quals, opt: RecOpt,
                paired: bool, bam_cap: int | None = None):
    """bsw_bam_records (host arrays): sam_text's arguments -> (the BAM alignment blocks as bytes, bam_off int64
    [n_rec + 1]).  A bam_cap below what is needed raises BswError with .needed and .bam_off set."""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    rec_first = np.ascontiguousarray(rec_first, dtype=np.int32)
    aln = np.ascontiguousarray(aln, dtype=ALN_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    md = np.ascontiguousarray(md, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    quals = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
    nm, nm_off = _names_host(names)
    n_reads = len(read_len)
    assert len(names) == (n_reads // 2 if paired else n_reads) and (quals is None or len(quals) == len(reads))
    cs = cigar.shape[1] if cigar.ndim == 2 else 1
    ms = md.shape[1] if md.ndim == 2 else 1
    if bam_cap is None:         # the text's bound holds: no field is longer in binary than printed
        per = 256 + 160 + 2 * int(read_len.max(initial=0)) + ms + 12 * cs * 16
        bam_cap = per * max(len(recs), 1)
    bam = np.zeros(max(bam_cap, 1), dtype=np.uint8)
    bam_off = np.zeros(len(recs) + 1, dtype=np.int64)
    n_bytes = ctypes.c_int64(-1)
    rc = hip_lib().bsw_bam_records(engine._ctx, ctypes.byref(opt), _ptr(recs), _ptr(rec_first), len(recs), _ptr(aln),
                                   _ptr(cigar), cs, _ptr(md), ms, len(aln), _ptr(reads), _ptr(read_off), _ptr(read_len),
                                   n_reads, _ptr(nm), _ptr(nm_off), _ptr(quals) if quals is not None else None,
                                   int(paired), _ptr(bam), _ptr(bam_off), bam_cap, ctypes.byref(n_bytes))
    if rc != 0:
        try:
            _raise_needed(rc, n_bytes)
        except BswError as e:
            e.bam_off = bam_off
            raise
    return bam[:n_bytes.value].tobytes(), bam_off


def bam_records_resident(engine, d_recs: int, d_rec_first: int, n_rec: int, d_aln: int, d_cigar: int, cigar_stride: int,
                         d_md: int, md_stride: int, n_aln: int, d_reads: int, d_off: int, d_len: int, n_reads: int,
                         d_names: int, d_name_off: int, d_quals: int, paired: bool, d_bam: int, d_bam_off: int,
                         bam_cap: int, opt: RecOpt, stream: int = 0) -> int:
    """bsw_bam_records_resident: every array a device pointer.  Returns n_bytes."""
    V = ctypes.c_void_p
    n_bytes = ctypes.c_int64(-1)
    rc = hip_lib().bsw_bam_records_resident(engine._ctx, ctypes.byref(opt), V(d_recs or None), V(d_rec_first or None),
                                            n_rec, V(d_aln or None), V(d_cigar or None), cigar_stride, V(d_md or None),
                                            md_stride, n_aln, V(d_reads or None), V(d_off or None), V(d_len or None),
                                            n_reads, V(d_names or None), V(d_name_off), V(d_quals or None), int(paired),
                                            V(d_bam or None), V(d_bam_off), bam_cap, ctypes.byref(n_bytes),
                                            V(stream or None))
    if rc != 0:
        _raise_needed(rc, n_bytes)
    return n_bytes.value


def bam_header(engine, opt: RecOpt, sam_text: bytes = b"") -> bytes:
    """bsw_bam_header: the uncompressed header block for the engine's contig table (or opt.rname / opt.l_pac)"""
    n_bytes = ctypes.c_int64(-1)
    L = hip_lib()
    rc = L.bsw_bam_header(engine._ctx, ctypes.byref(opt), sam_text or None, len(sam_text), None, 0, ctypes.byref(n_bytes))
    if rc != -34 or n_bytes.value <= 0:
        _check(rc)
    out = np.zeros(n_bytes.value, dtype=np.uint8)
    _check(L.bsw_bam_header(engine._ctx, ctypes.byref(opt), sam_text or None, len(sam_text), _ptr(out), len(out),
                            ctypes.byref(n_bytes)))
    return out[:n_bytes.value].tobytes()


def bam_last_stats(engine) -> BamStats:
    st = BamStats()
    _check(hip_lib().bsw_bam_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- BGZF (bsw_bgzf.h)
class BgzfOpt(ctypes.Structure):
    _fields_ = [("level", ctypes.c_int32), ("block_bytes", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_int32), ("base_coffset", ctypes.c_int64)]


class BgzfStats(ctypes.Structure):
    _fields_ = [("n_blocks", ctypes.c_int32), ("n_stored", ctypes.c_int32), ("n_fixed", ctypes.c_int32),
                ("n_dynamic", ctypes.c_int32), ("n_in", ctypes.c_int64), ("n_out", ctypes.c_int64),
                ("deflate_ms", ctypes.c_float), ("pack_ms", ctypes.c_float)]


def bgzf_opt(**kw) -> BgzfOpt:
    """bsw_bgzf_opt_default, then the given fields (level, block_bytes, flags, base_coffset)"""
    o = BgzfOpt()
    hip_lib().bsw_bgzf_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        if k not in ("level", "block_bytes", "flags", "base_coffset"):
            raise TypeError(f"bgzf_opt: no field '{k}'")
        setattr(o, k, v)
    return o


def bgzf_blocks(n_in: int, opt: BgzfOpt) -> int:
    return -(-n_in // opt.block_bytes)


def bgzf_bound(n_in: int, opt: BgzfOpt) -> int:
    """bytes that hold any input of n_in bytes: every block stored, the EOF marker"""
    return n_in + 31 * bgzf_blocks(n_in, opt) + 28


def bgzf(engine, data, opt: BgzfOpt | None = None, rec_off=None, out_cap: int | None = None, blk_cap: int | None = None):
    """bsw_bgzf (host arrays): bytes -> (the BGZF blocks as bytes, blk_off int64 [n_blocks + 1], voff int64 [n_rec] or
    None).  rec_off: n_rec + 1 offsets into data.  An out_cap below what is needed raises BswError with .needed,
    .blk_off and .voff set; a blk_cap below n_blocks + 1 with .n_blocks set."""
    opt = bgzf_opt() if opt is None else opt
    data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                                dtype=np.uint8)
    n_rec = 0 if rec_off is None else len(rec_off) - 1
    rec_off = None if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.int64)
    nb = bgzf_blocks(len(data), opt)
    out_cap = bgzf_bound(len(data), opt) if out_cap is None else out_cap
    blk_cap = nb + 1 if blk_cap is None else blk_cap
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    blk_off = np.zeros(max(blk_cap, 1), dtype=np.int64)
    voff = np.zeros(max(n_rec, 1), dtype=np.int64)
    n_blocks, n_bytes = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = hip_lib().bsw_bgzf(engine._ctx, ctypes.byref(opt), _ptr(data), len(data), None if rec_off is None else _ptr(rec_off),
                            n_rec, _ptr(out), out_cap, _ptr(blk_off), blk_cap, _ptr(voff), ctypes.byref(n_blocks),
                            ctypes.byref(n_bytes))
    if rc != 0:
        try:
            _raise_needed(rc, n_bytes)
        except BswError as e:
            e.n_blocks, e.blk_off, e.voff = n_blocks.value, blk_off, voff[:n_rec]
            raise
    return out[:n_bytes.value].tobytes(), blk_off[:n_blocks.value + 1], (voff[:n_rec] if rec_off is not None else None)


def bgzf_resident(engine, d_in: int, n_in: int, d_rec_off: int, n_rec: int, d_out: int, out_cap: int, d_blk_off: int,
                  blk_cap: int, d_voff: int, opt: BgzfOpt, stream: int = 0):
    """bsw_bgzf_resident: every array a device pointer.  Returns (n_blocks, n_bytes)."""
    V = ctypes.c_void_p
    n_blocks, n_bytes = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = hip_lib().bsw_bgzf_resident(engine._ctx, ctypes.byref(opt), V(d_in or None), n_in, V(d_rec_off or None), n_rec,
                                     V(d_out or None), out_cap, V(d_blk_off or None), blk_cap, V(d_voff or None),
                                     ctypes.byref(n_blocks), ctypes.byref(n_bytes), V(stream or None))
    if rc != 0:
        try:
            _raise_needed(rc, n_bytes)
        except BswError as e:
            e.n_blocks = n_blocks.value
            raise
    return n_blocks.value, n_bytes.value


def bgzf_last_stats(engine) -> BgzfStats:
    st = BgzfStats()
    _check(hip_lib().bsw_bgzf_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- BAM sort and index (bsw_bamsort.h)
class BamsortOpt(ctypes.Structure):
    _fields_ = [("n_ref", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class BamsortStats(ctypes.Structure):
    _fields_ = [("n_rec", ctypes.c_int32), ("key_bits", ctypes.c_int32), ("n_bytes", ctypes.c_int64),
                ("key_ms", ctypes.c_float), ("sort_ms", ctypes.c_float), ("copy_ms", ctypes.c_float),
                ("index_ms", ctypes.c_float), ("n_bins", ctypes.c_int32), ("n_chunks", ctypes.c_int32),
                ("n_intv", ctypes.c_int64), ("n_no_coor", ctypes.c_int64), ("bai_bytes", ctypes.c_int64)]


def bamsort_opt(n_ref: int, flags: int = 0) -> BamsortOpt:
    return BamsortOpt(n_ref, flags)


def bam_sort(engine, bam, bam_off, n_ref: int, out_cap: int | None = None):
    """bsw_bam_sort (host arrays): BAM alignment blocks and their offsets [n_rec + 1] -> (the blocks in coordinate
    order as bytes, out_off int64 [n_rec + 1], perm int32 [n_rec]: the input index of output record i)"""
    bam = np.ascontiguousarray(np.frombuffer(bam, dtype=np.uint8) if isinstance(bam, (bytes, bytearray)) else bam, dtype=np.uint8)
    bam_off = np.ascontiguousarray(bam_off, dtype=np.int64)
    n_rec = len(bam_off) - 1
    out_cap = len(bam) if out_cap is None else out_cap
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    out_off, perm = np.zeros(n_rec + 1, dtype=np.int64), np.zeros(max(n_rec, 1), dtype=np.int32)
    opt = bamsort_opt(n_ref)
    _check(hip_lib().bsw_bam_sort(engine._ctx, ctypes.byref(opt), _ptr(bam), _ptr(bam_off), n_rec, _ptr(out), out_cap,
                                  _ptr(out_off), _ptr(perm)))
    return out[:int(bam_off[n_rec])].tobytes(), out_off, perm[:n_rec]


def bam_sort_resident(engine, d_bam: int, d_bam_off: int, n_rec: int, d_out: int, out_cap: int, d_out_off: int, d_perm: int,
                      opt: BamsortOpt, stream: int = 0) -> None:
    """bsw_bam_sort_resident: every array a device pointer"""
    V = ctypes.c_void_p
    _check(hip_lib().bsw_bam_sort_resident(engine._ctx, ctypes.byref(opt), V(d_bam or None), V(d_bam_off or None), n_rec,
                                           V(d_out or None), out_cap, V(d_out_off or None), V(d_perm or None),
                                           V(stream or None)))


def bam_index(engine, bam, bam_off, voff, end_voff: int, ref_len, bai_cap: int | None = None) -> bytes:
    """bsw_bam_index (host arrays): the sorted blocks, their offsets and virtual offsets -> the .bai file's bytes.
    bai_cap=None: one call with no room that says how many bytes are needed, then the call with exactly those.  A
    bai_cap below what is needed raises BswError with .needed set."""
    bam = np.ascontiguousarray(np.frombuffer(bam, dtype=np.uint8) if isinstance(bam, (bytes, bytearray)) else bam, dtype=np.uint8)
    bam_off = np.ascontiguousarray(bam_off, dtype=np.int64)
    voff = np.ascontiguousarray(voff, dtype=np.int64)
    ref_len = np.ascontiguousarray(ref_len, dtype=np.int32)
    n_rec = len(bam_off) - 1
    opt = bamsort_opt(len(ref_len))
    n_bytes = ctypes.c_int64(-1)

    def call(cap):
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        rc = hip_lib().bsw_bam_index(engine._ctx, ctypes.byref(opt), _ptr(ref_len), _ptr(bam), _ptr(bam_off), n_rec,
                                     _ptr(voff), end_voff, _ptr(out), cap, ctypes.byref(n_bytes))
        if rc != 0:
            _raise_needed(rc, n_bytes)
        return out[:n_bytes.value].tobytes()

    if bai_cap is None:
        try:
            return call(0)          # (no index is 0 bytes long)
        except BswError as e:
            if getattr(e, "needed", -1) <= 0:
                raise
            bai_cap = e.needed
    return call(bai_cap)


def bam_index_resident(engine, ref_len, d_bam: int, d_bam_off: int, n_rec: int, d_voff: int, end_voff: int, d_bai: int,
                       bai_cap: int, stream: int = 0) -> int:
    """bsw_bam_index_resident: every array but ref_len a device pointer.  Returns n_bytes; a short bai_cap raises
    BswError with .needed set."""
    V = ctypes.c_void_p
    ref_len = np.ascontiguousarray(ref_len, dtype=np.int32)
    opt = bamsort_opt(len(ref_len))
    n_bytes = ctypes.c_int64(-1)
    rc = hip_lib().bsw_bam_index_resident(engine._ctx, ctypes.byref(opt), _ptr(ref_len), V(d_bam or None), V(d_bam_off or None),
                                          n_rec, V(d_voff or None), end_voff, V(d_bai or None), bai_cap, ctypes.byref(n_bytes),
                                          V(stream or None))
    if rc != 0:
        _raise_needed(rc, n_bytes)
    return n_bytes.value


def bamsort_last_stats(engine) -> BamsortStats:
    st = BamsortStats()
    _check(hip_lib().bsw_bamsort_last_stats(engine._ctx, ctypes.byref(st)))
    return st


# ---------------------------------------------------------------- duplicate marking (bsw_markdup.h)
class MarkdupOpt(ctypes.Structure):
    _fields_ = [("l_pac", ctypes.c_int64), ("min_qual", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class MarkdupStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("n_reads", "n_cand", "n_pair_cand", "n_dup_pairs", "n_dup_frag", "n_dup_frag_by_pair",
                                              "n_pair_sets", "n_end_sets", "n_flagged", "pair_key_bits", "end_key_bits",
                                              "pair_route", "end_route")] + \
               [(k, ctypes.c_float) for k in ("score_ms", "key_ms", "sort_ms", "mark_ms")] + [("reserved", ctypes.c_int32)]


def markdup_opt(l_pac: int, min_qual: int | None = None, flags: int = 0) -> MarkdupOpt:
    """bsw_markdup_opt_default with l_pac set; min_qual=None keeps the default (15)"""
    o = MarkdupOpt()
    hip_lib().bsw_markdup_opt_default(ctypes.byref(o))
    o.l_pac, o.flags = l_pac, flags
    if min_qual is not None:
        o.min_qual = min_qual
    return o


def mark_duplicates(engine, recs, rec_first, aln, cigar, read_off, read_len, quals, paired: bool, opt: MarkdupOpt):
    """bsw_mark_duplicates (host arrays): records, alignments and CIGAR rows as bsw_records left them, the reads'
    offsets and lengths, quals (uint8, parallel to the reads) or None -> (the records with 0x400 set or cleared,
    dup uint8 [n_reads])"""
    recs = np.array(recs, dtype=REC_DTYPE, copy=True)
    rec_first = np.ascontiguousarray(rec_first, dtype=np.int32)
    aln = np.ascontiguousarray(aln, dtype=ALN_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    n_reads = len(read_len)
    stride = cigar.shape[1] if cigar.ndim == 2 else 1
    q = None if quals is None else np.ascontiguousarray(
        np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals, dtype=np.uint8)
    dup = np.zeros(max(n_reads, 1), dtype=np.uint8)
    _check(hip_lib().bsw_mark_duplicates(engine._ctx, ctypes.byref(opt), _ptr(recs), _ptr(rec_first), len(recs), _ptr(aln),
                                         _ptr(cigar), stride, len(aln), _ptr(read_off), _ptr(read_len), n_reads,
                                         None if q is None else _ptr(q), 0 if q is None else len(q), int(bool(paired)), _ptr(dup)))
    return recs, dup[:n_reads]


def mark_duplicates_resident(engine, d_recs: int, d_rec_first: int, n_rec: int, d_aln: int, d_cigar: int, cigar_stride: int,
                             n_aln: int, d_read_off: int, d_read_len: int, n_reads: int, d_quals: int, quals_len: int,
                             paired: bool, d_dup: int, opt: MarkdupOpt, stream: int = 0) -> None:
    """bsw_mark_duplicates_resident: every array a device pointer; d_recs is marked in place"""
    V = ctypes.c_void_p
    _check(hip_lib().bsw_mark_duplicates_resident(engine._ctx, ctypes.byref(opt), V(d_recs or None), V(d_rec_first or None), n_rec,
                                                  V(d_aln or None), V(d_cigar or None), cigar_stride, n_aln, V(d_read_off or None),
                                                  V(d_read_len or None), n_reads, V(d_quals or None), quals_len,
                                                  int(bool(paired)), V(d_dup or None), V(stream or None)))


def markdup_last_stats(engine) -> MarkdupStats:
    st = MarkdupStats()
    _check(hip_lib().bsw_markdup_last_stats(engine._ctx, ctypes.byref(st)))
    return st


class MatesCfg(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("read_len", ctypes.c_int32), ("win_len", ctypes.c_int32),
                ("a", ctypes.c_int32), ("min_seed", ctypes.c_int32), ("p_true", ctypes.c_double),
                ("p_sub", ctypes.c_double), ("p_indel", ctypes.c_double)]


def mates_cfg(**kw) -> MatesCfg:
    c = MatesCfg()
    synth_lib().bsw_mates_default(ctypes.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def synth_mates(ref: np.ndarray, n: int, base: int = 0, cfg: MatesCfg | None = None):
    """Mate-rescue jobs against ref (bsw_synth_mates): (pairs, qer); seqBufRef is ref itself."""
    cfg = cfg if cfg is not None else mates_cfg()
    pairs = np.zeros(n, dtype=SEQPAIR_DTYPE)
    qer = np.zeros(max(1, n * cfg.read_len), dtype=np.uint8)
    r = synth_lib().bsw_synth_mates(ctypes.byref(cfg), _ptr(ref), len(ref), base, n, _ptr(pairs), _ptr(qer))
    if r < 0:
        raise BswError("bsw_synth_mates: reference too short for the window")
    return pairs, qer


class GlobalsCfg(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("read_len", ctypes.c_int32), ("w_cap", ctypes.c_int32),
                ("a", ctypes.c_int32), ("o_del", ctypes.c_int32), ("e_del", ctypes.c_int32),
                ("o_ins", ctypes.c_int32), ("e_ins", ctypes.c_int32), ("p_sub", ctypes.c_double),
                ("p_indel", ctypes.c_double)]


def globals_cfg(**kw) -> GlobalsCfg:
    c = GlobalsCfg()
    synth_lib().bsw_globals_default(ctypes.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def synth_globals(ref: np.ndarray, n: int, base: int = 0, cfg: GlobalsCfg | None = None):
    """ksw_global2 jobs shaped like bwa_gen_cigar2's (bsw_synth_globals): (pairs, qer); seqBufRef
    is ref itself, h0 = the band w."""
    cfg = cfg if cfg is not None else globals_cfg()
    pairs = np.zeros(n, dtype=SEQPAIR_DTYPE)
    qer = np.zeros(max(1, n * cfg.read_len), dtype=np.uint8)
    r = synth_lib().bsw_synth_globals(ctypes.byref(cfg), _ptr(ref), len(ref), base, n, _ptr(pairs), _ptr(qer))
    if r < 0:
        raise BswError("bsw_synth_globals: reference too short for the read length")
    return pairs, qer


# ---- include/bsw_fmi.h: FM-index SMEM seeding

BWTINTV_DTYPE = np.dtype([("k", "<u8"), ("l", "<u8"), ("s", "<u8"), ("info", "<u8")])   # bsw_bwtintv_t
assert BWTINTV_DTYPE.itemsize == 32


class MemOpt(ctypes.Structure):
    _fields_ = [("min_seed_len", ctypes.c_int32), ("split_width", ctypes.c_int32),
                ("max_mem_intv", ctypes.c_int32), ("split_factor", ctypes.c_float)]


class FmiInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("sentinel", ctypes.c_int64), ("count", ctypes.c_int64 * 5),
                ("device_bytes", ctypes.c_int64), ("build_s", ctypes.c_float)]


def mem_opt(**kw) -> MemOpt:
    o = MemOpt()
    hip_lib().bsw_mem_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


FMI_GPU_BUILD, FMI_WIDE, FMI_NO_TEXT, FMI_PLAIN_ENT = 1, 2, 4, 8


class Fmi:
    """One resident FM-index (bsw_fmi_t) of ref + reverse-complement(ref) on `device`;
    flags: FMI_GPU_BUILD / FMI_WIDE / FMI_NO_TEXT (bsw_fmi_build2), None: the library's choice."""

    def __init__(self, ref: np.ndarray, device: int = 0, flags: int | None = None):
        self.ref = np.ascontiguousarray(ref, dtype=np.uint8)
        self._f = ctypes.c_void_p()
        if flags is None:
            _check(hip_lib().bsw_fmi_build(_ptr(self.ref), len(self.ref), device, ctypes.byref(self._f)))
        else:
            _check(hip_lib().bsw_fmi_build2(_ptr(self.ref), len(self.ref), device, flags, ctypes.byref(self._f)))

    def close(self):
        if self._f:
            hip_lib().bsw_fmi_destroy(self._f)
            self._f = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_contigs(self, lens=()):
        """bsw_fmi_set_contigs (include/bsw_contigs.h): the contig lengths for mem_chain_device; none removes them."""
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        _check(hip_lib().bsw_fmi_set_contigs(self._f, len(lens), _ptr(lens) if len(lens) else None))

    def check(self) -> int:
        """bsw_fmi_check: number of violated index invariants (0 = consistent)"""
        bad = ctypes.c_int64(-1)
        _check(hip_lib().bsw_fmi_check(self._f, ctypes.byref(bad)))
        return bad.value

    def info(self) -> FmiInfo:
        i = FmiInfo()
        _check(hip_lib().bsw_fmi_get_info(self._f, ctypes.byref(i)))
        return i

    def sa(self) -> np.ndarray:
        a = np.zeros(self.info().n + 1, dtype=np.int64)
        _check(hip_lib().bsw_fmi_copy_sa(self._f, _ptr(a)))
        return a

    def bwt(self) -> np.ndarray:
        a = np.zeros(self.info().n + 1, dtype=np.uint8)
        _check(hip_lib().bsw_fmi_copy_bwt(self._f, _ptr(a)))
        return a

    def collect_intv(self, reads, read_off, read_len, cap: int = 256, opt: MemOpt | None = None, strict=True):
        """bsw_mem_collect_intv (host buffers) -> (intervals [n, cap], counts [n])"""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        n = len(read_len)
        out = np.zeros((n, cap), dtype=BWTINTV_DTYPE)
        cnt = np.zeros(n, dtype=np.int32)
        o = opt if opt is not None else mem_opt()
        rc = hip_lib().bsw_mem_collect_intv(self._f, ctypes.byref(o), _ptr(reads), _ptr(read_off), _ptr(read_len),
                                            n, _ptr(out), cap, _ptr(cnt))
        if strict or rc != -34:
            _check(rc)
        return out, cnt

    def collect_intv_device(self, d_reads: int, d_off: int, d_len: int, n: int, max_len: int, d_mems: int, cap: int,
                            d_cnt: int, opt: MemOpt | None = None, stream: int = 0) -> int:
        o = opt if opt is not None else mem_opt()
        return hip_lib().bsw_mem_collect_intv_device(self._f, ctypes.byref(o), ctypes.c_void_p(d_reads),
                                                     ctypes.c_void_p(d_off), ctypes.c_void_p(d_len), n, max_len,
                                                     ctypes.c_void_p(d_mems), cap, ctypes.c_void_p(d_cnt),
                                                     ctypes.c_void_p(stream or None))

    def sa_device(self, d_k: int, n: int, d_pos: int, stream: int = 0):
        _check(hip_lib().bsw_fmi_sa_device(self._f, ctypes.c_void_p(d_k), n, ctypes.c_void_p(d_pos),
                                           ctypes.c_void_p(stream or None)))

    def last_kernel_ms(self) -> float:
        v = ctypes.c_float()
        _check(hip_lib().bsw_fmi_last_kernel_ms(self._f, ctypes.byref(v)))
        return v.value

    def last_launch(self) -> tuple:
        """bsw_fmi_last_launch: (SMEM kernel launches, scratch entry bytes) of the last seeding call"""
        n, e = ctypes.c_int32(), ctypes.c_int32()
        _check(hip_lib().bsw_fmi_last_launch(self._f, ctypes.byref(n), ctypes.byref(e)))
        return n.value, e.value

    def mem_chain_device(self, d_len: int, n: int, d_mems: int, cap: int, d_cnt: int, d_seeds: int, d_sr: int,
                         d_sc: int, seed_cap: int, opt: "ChainOpt | None" = None, stream: int = 0):
        """bsw_mem_chain_device -> (status, seeds needed / written)"""
        o = opt if opt is not None else chain_opt()
        ns = ctypes.c_int64(0)
        rc = hip_lib().bsw_mem_chain_device(self._f, ctypes.byref(o), ctypes.c_void_p(d_len), n,
                                            ctypes.c_void_p(d_mems), cap, ctypes.c_void_p(d_cnt),
                                            ctypes.c_void_p(d_seeds or None), ctypes.c_void_p(d_sr or None),
                                            ctypes.c_void_p(d_sc or None), seed_cap, ctypes.byref(ns),
                                            ctypes.c_void_p(stream or None))
        return rc, ns.value


class ChainOpt(ctypes.Structure):
    """Mirror of bsw_chain_opt_t (include/bsw_fmi.h)."""
    _fields_ = [("max_occ", ctypes.c_int32), ("w", ctypes.c_int32), ("max_chain_gap", ctypes.c_int32),
                ("min_chain_weight", ctypes.c_int32), ("min_seed_len", ctypes.c_int32),
                ("max_chain_extend", ctypes.c_int32), ("drop_ratio", ctypes.c_float), ("mask_level", ctypes.c_float)]


def chain_opt(**kw) -> ChainOpt:
    o = ChainOpt()
    hip_lib().bsw_chain_opt_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def seed_and_chain(fmi: Fmi, d_reads, read_off, read_len, cap: int = 256, mopt=None, copt=None):
    """The GPU seeding front end of mem_align1_core over resident reads: bsw_mem_collect_intv_device
    -> bsw_mem_chain_device.  d_reads: a hiprt.DeviceBuffer of the reads.  Returns host copies
    (seeds, seed_read, seed_chain) and the device buffers holding them (d_seeds, d_sr, d_sc)."""
    import hiprt
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    n = len(read_len)
    d_off, d_len = hiprt.DeviceBuffer.from_array(read_off), hiprt.DeviceBuffer.from_array(read_len)
    d_mems = hiprt.DeviceBuffer(max(1, n * cap) * BWTINTV_DTYPE.itemsize)
    d_cnt = hiprt.DeviceBuffer(max(1, n) * 4)
    _check(fmi.collect_intv_device(d_reads.ptr, d_off.ptr, d_len.ptr, n, int(read_len.max(initial=0)), d_mems.ptr, cap,
                                   d_cnt.ptr, mopt))
    rc, need = fmi.mem_chain_device(d_len.ptr, n, d_mems.ptr, cap, d_cnt.ptr, 0, 0, 0, 0, copt)
    if rc not in (0, -34):
        _check(rc)
    d_seeds = hiprt.DeviceBuffer(max(1, need) * SEED_DTYPE.itemsize)
    d_sr, d_sc = hiprt.DeviceBuffer(max(1, need) * 4), hiprt.DeviceBuffer(max(1, need) * 4)
    rc, got = fmi.mem_chain_device(d_len.ptr, n, d_mems.ptr, cap, d_cnt.ptr, d_seeds.ptr, d_sr.ptr, d_sc.ptr, need, copt)
    _check(rc)
    assert got == need
    seeds = d_seeds.download(np.zeros(need, dtype=SEED_DTYPE)) if need else np.zeros(0, SEED_DTYPE)
    sr = d_sr.download(np.zeros(need, dtype=np.int32)) if need else np.zeros(0, np.int32)
    sc = d_sc.download(np.zeros(need, dtype=np.int32)) if need else np.zeros(0, np.int32)
    return (seeds, sr, sc), (d_seeds, d_sr, d_sc), (d_off, d_len)
