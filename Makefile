# Native build of the seed-extension engine (gfx950 only) and its test infrastructure.
#   make            -> product library + tools + oracle
#   make product    -> bwa-mem2-arm_amd/lib/libbsw_hip.so   (HIP kernels + C ABI)
#   make oracle     -> oracle/liboracle.so                  (CPU oracle + SSE4.1 baseline; tests only)
PKG      := bwa-mem2-arm_amd
CSRC     := $(PKG)/csrc
LIBDIR   := $(PKG)/lib
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function \
            -munsafe-fp-atomics -Iinclude
CFLAGS   ?= -O3 -fPIC -Wall -Iinclude

PRODUCT  := $(LIBDIR)/libbsw_hip.so
SYNTH    := $(LIBDIR)/libbsw_synth.so
SHIMTEST := $(LIBDIR)/bsw_shim_example
ORACLE   := oracle/liboracle.so

HIP_HDRS := $(CSRC)/bsw_devcache.h $(CSRC)/bsw_pool.h $(CSRC)/bsw_kernels.h $(CSRC)/bsw_mate_k.h include/bsw_mate.h $(CSRC)/bsw_global_k.h include/bsw_global.h $(CSRC)/bsw_ext_k.h $(CSRC)/bsw_aln_k.h include/bsw_aln.h $(CSRC)/bsw_sel_k.h $(CSRC)/bsw_sel_dev.h include/bsw_sel.h $(CSRC)/bsw_pe_k.h include/bsw_pe.h $(CSRC)/bsw_matesw_k.h include/bsw_matesw.h $(CSRC)/bsw_rec_k.h include/bsw_rec.h include/bsw_bam.h $(CSRC)/bsw_bgzf_k.h include/bsw_bgzf.h $(CSRC)/bsw_bamsort_k.h include/bsw_bamsort.h $(CSRC)/bsw_markdup_k.h include/bsw_markdup.h $(CSRC)/bsw_wave.h $(CSRC)/bsw_pc_rules.h $(CSRC)/bsw_pc_group.h $(CSRC)/bsw_pc_scan.h $(CSRC)/bsw_formulas.h $(CSRC)/bsw_contig_seg.h include/bsw_contigs.h $(CSRC)/bsw_stage_k.h $(CSRC)/bsw_internal.h $(CSRC)/bsw_stage_plan.h $(CSRC)/bsw_engine.h $(CSRC)/bsw_sort.h $(CSRC)/bsw_fmi_internal.h include/bsw.h include/bsw_seqpair.h include/bsw_ext.h include/bsw_batch.h include/bsw_fmi.h include/bsw_fmi_launch.h

# the product's objects; the experiment libraries below are this list with one object swapped
OBJS := $(addprefix $(LIBDIR)/,bsw_kernels.o bsw_pc.o bsw_wv.o bsw_gq.o bsw_mate.o bsw_global.o bsw_ext_dev.o bsw_aln.o bsw_sel.o bsw_pe.o bsw_matesw.o bsw_rec.o bsw_bgzf.o bsw_bamsort.o bsw_markdup.o bsw_stage.o \
          bsw_fmi.o bsw_fmi_build.o bsw_memchain.o bsw_chain.o bsw_dispatch.o bsw_sort.o bsw_pipeline.o bsw_host.o bsw_stages.o bsw_ext.o \
          bsw_pack.o bsw_devcache.o bsw_batch.o)
LINK  = $(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(1) -lpthread

all: product synth oracle percall

PERCALL := $(LIBDIR)/percall_bench
percall: $(PERCALL)
$(PERCALL): tools/percall_bench.cpp $(PRODUCT) $(SYNTH) include/bsw.h
	g++ -O2 -std=c++17 -pthread -Iinclude -o $@ $< $(PRODUCT) $(SYNTH) -Wl,-rpath,'$$ORIGIN'

product: $(PRODUCT)
synth: $(SYNTH)
oracle: $(ORACLE)

$(LIBDIR):
	mkdir -p $(LIBDIR)

$(LIBDIR)/%.o: $(CSRC)/%.hip $(HIP_HDRS) | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# hipcc-compiled .cpp (bsw_host.cpp and bsw_stages.cpp as HIP; bsw_ext.cpp and bsw_pack.cpp have g++
# rules of their own below)
$(LIBDIR)/%.o: $(CSRC)/%.cpp $(HIP_HDRS) | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(XHIP) -c $< -o $@
$(LIBDIR)/bsw_host.o $(LIBDIR)/bsw_stages.o: XHIP := -x hip

$(LIBDIR)/bsw_ext.o: $(CSRC)/bsw_ext.cpp $(HIP_HDRS) | $(LIBDIR)
	g++ -O3 -std=c++17 -fPIC -Wall -Iinclude -c $< -o $@

$(LIBDIR)/bsw_pack.o: $(CSRC)/bsw_pack.cpp $(CSRC)/bsw_internal.h $(CSRC)/bsw_stage_plan.h | $(LIBDIR)
	g++ -O3 -std=c++17 -fPIC -Wall -Iinclude -c $< -o $@

$(LIBDIR)/bsw_batch.o: $(CSRC)/bsw_batch.c include/bsw_batch.h include/bsw.h | $(LIBDIR)
	gcc $(CFLAGS) -std=c11 -c $< -o $@

$(PRODUCT): $(OBJS)
	$(call LINK,$^)

$(SYNTH): $(CSRC)/bsw_synth.c include/bsw_seqpair.h | $(LIBDIR)
	gcc $(CFLAGS) -shared -o $@ $<

ORACLE_SRCS := oracle/ksw_ext_ref.c oracle/bsw_sse41.c oracle/bsw_avx512.c oracle/ext_ref.c oracle/ksw_align_ref.c oracle/ksw_global_ref.c oracle/fmi_ref.c oracle/chain_ref.c
$(ORACLE): $(ORACLE_SRCS) oracle/bsw_simd_batch.inc oracle/bsw_simd_common.h include/bsw_seqpair.h include/bsw_ext.h include/bsw_fmi.h
	gcc $(CFLAGS) -msse4.1 -shared -o $@ $(ORACLE_SRCS) -lpthread

# the serial model of the BAM sort and index kernels (tools/bamsort_model.cpp over bsw_bamsort_k.h; no GPU), and the same
# program under AddressSanitizer + UBSan: stand-alone, run over files (tests/test_bamsort.py writes them)
BAMSORT_MODEL := $(LIBDIR)/bamsort_model
bamsort-model: $(BAMSORT_MODEL) $(BAMSORT_MODEL)_asan
$(BAMSORT_MODEL): tools/bamsort_model.cpp $(CSRC)/bsw_bamsort_k.h | $(LIBDIR)
	g++ -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<
$(BAMSORT_MODEL)_asan: tools/bamsort_model.cpp $(CSRC)/bsw_bamsort_k.h | $(LIBDIR)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$(CSRC) -o $@ $<

# the serial model of the duplicate marking (tools/markdup_model.cpp over bsw_markdup_k.h; no GPU), and the same program
# under AddressSanitizer + UBSan: stand-alone, run over files (tests/test_markdup.py writes them)
MARKDUP_MODEL := $(LIBDIR)/markdup_model
MARKDUP_DEPS  := tools/markdup_model.cpp $(CSRC)/bsw_markdup_k.h $(CSRC)/bsw_contig_seg.h $(CSRC)/bsw_formulas.h include/bsw_rec.h
markdup-model: $(MARKDUP_MODEL) $(MARKDUP_MODEL)_asan
$(MARKDUP_MODEL): $(MARKDUP_DEPS) | $(LIBDIR)
	g++ -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<
$(MARKDUP_MODEL)_asan: $(MARKDUP_DEPS) | $(LIBDIR)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$(CSRC) -o $@ $<

clean:
	rm -f $(LIBDIR)/*.o $(LIBDIR)/*.so $(ORACLE) $(BAMSORT_MODEL) $(BAMSORT_MODEL)_asan $(MARKDUP_MODEL) $(MARKDUP_MODEL)_asan

# experiment build: pc_kernel group-path counters (tools/pc_stats.py), never loaded by the product
STATSLIB := $(LIBDIR)/libbsw_hip_stats.so
stats: $(STATSLIB)
$(LIBDIR)/bsw_pc_stats.o: $(CSRC)/bsw_pc.hip $(HIP_HDRS) | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -DBSW_PC_STATS -c $< -o $@
$(STATSLIB): $(subst bsw_pc.o,bsw_pc_stats.o,$(OBJS))
	$(call LINK,$^)

# experiment builds: the product with one file compiled under AB_FLAGS (same-box A/B runs:
# tools/ab_lib.sh) -- ab: bsw_pc.hip -> libbsw_hip_ab.so; abhost: bsw_pipeline.hip (host pipeline,
# host_shard) -> libbsw_hip_abhost.so; abfmi: bsw_fmi.hip (SMEM walk) -> libbsw_hip_abfmi.so; abrec: bsw_rec.hip
# (lanes per record of the text kernel, -DBSW_REC_TEXT_GROUP=N, and of the BAM kernel, -DBSW_REC_BAM_GROUP=N)
# -> libbsw_hip_abrec.so; absort: bsw_sort.hip (-DBSW_SORT_ONESWEEP: the library's radix route) -> libbsw_hip_absort.so;
# abbgzf: bsw_bgzf.hip (-DBSW_BGZF_PACK_BYTES: byte stores in the compaction) -> libbsw_hip_abbgzf.so;
# abmarkdup: bsw_markdup.hip (lanes per read of the score kernel, -DBSW_MD_SCORE_GROUP=N) -> libbsw_hip_abmarkdup.so
AB_FLAGS ?=
AB_SRC_ab := bsw_pc
AB_SRC_abhost := bsw_pipeline
AB_SRC_abfmi := bsw_fmi
AB_SRC_abrec := bsw_rec
AB_SRC_absort := bsw_sort
AB_SRC_abbgzf := bsw_bgzf
AB_SRC_abmarkdup := bsw_markdup
ab abhost abfmi abrec absort abbgzf abmarkdup:
	$(HIPCC) $(HIPFLAGS) $(AB_FLAGS) -c $(CSRC)/$(AB_SRC_$@).hip -o $(LIBDIR)/$(AB_SRC_$@)_ab.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(LIBDIR)/libbsw_hip_$@.so $(subst $(AB_SRC_$@).o,$(AB_SRC_$@)_ab.o,$(OBJS)) -lpthread

.PHONY: all product synth oracle percall clean stats ab abfmi abhost abrec absort abbgzf abmarkdup bamsort-model markdup-model

# host sanitizer build: AddressSanitizer + UBSan over the host C / C++ of the
# product (bsw_pack.cpp, bsw_ext.cpp, bsw_batch.c, bsw_synth.c) and the oracle, driven by
# tools/asan/asan_driver.cpp with an oracle-backed engine stub (no GPU).  Log: tools/asan/asan.log
ASAN_DIR   := tools/asan
ASAN_FLAGS := -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g -O1 -Iinclude
ASAN_BIN   := $(ASAN_DIR)/asan_driver
ASAN_C     := $(CSRC)/bsw_batch.c $(CSRC)/bsw_synth.c oracle/ksw_ext_ref.c oracle/ext_ref.c oracle/ksw_align_ref.c oracle/ksw_global_ref.c oracle/fmi_ref.c oracle/chain_ref.c
ASAN_SSE   := oracle/bsw_sse41.c oracle/bsw_avx512.c
ASAN_CXX   := $(ASAN_DIR)/asan_driver.cpp $(ASAN_DIR)/engine_stub.cpp $(CSRC)/bsw_ext.cpp $(CSRC)/bsw_pack.cpp
$(ASAN_BIN): $(ASAN_C) $(ASAN_SSE) oracle/bsw_simd_batch.inc oracle/bsw_simd_common.h $(ASAN_CXX) $(CSRC)/bsw_internal.h $(CSRC)/bsw_stage_plan.h $(CSRC)/bsw_formulas.h include/bsw_ext.h include/bsw_fmi.h
	mkdir -p $(ASAN_DIR)/obj
	for f in $(ASAN_C); do gcc $(ASAN_FLAGS) -std=gnu11 -c $$f -o $(ASAN_DIR)/obj/$$(basename $$f).o || exit 1; done
	for f in $(ASAN_SSE); do gcc $(ASAN_FLAGS) -std=gnu11 -msse4.1 -c $$f -o $(ASAN_DIR)/obj/$$(basename $$f).o || exit 1; done
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $(ASAN_CXX) $(ASAN_DIR)/obj/*.o -lpthread
asan: $(ASAN_BIN)
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
	  ./$(ASAN_BIN) > $(ASAN_DIR)/asan.log 2>&1; rc=$$?; cat $(ASAN_DIR)/asan.log; exit $$rc
# the CPU test suite (-m "not gpu") against sanitized builds of the oracle and the synthetic
# generator (LD_PRELOAD of the sanitizer runtimes into python; leak checks off: the interpreter
# keeps its arenas).  Log: tools/asan/asan_suite.log
ASAN_ORACLE := $(ASAN_DIR)/liboracle_asan.so
ASAN_SYNTH  := $(ASAN_DIR)/libbsw_synth_asan.so
$(ASAN_ORACLE): $(ORACLE_SRCS) oracle/bsw_simd_batch.inc oracle/bsw_simd_common.h include/bsw_seqpair.h include/bsw_ext.h include/bsw_fmi.h
	mkdir -p $(ASAN_DIR)
	gcc $(ASAN_FLAGS) -fPIC -msse4.1 -shared -o $@ $(ORACLE_SRCS) -lpthread
$(ASAN_SYNTH): $(CSRC)/bsw_synth.c include/bsw_seqpair.h
	mkdir -p $(ASAN_DIR)
	gcc $(ASAN_FLAGS) -fPIC -shared -o $@ $(CSRC)/bsw_synth.c
asan-suite: $(ASAN_ORACLE) $(ASAN_SYNTH)
	LD_PRELOAD="$$(gcc -print-file-name=libasan.so) $$(gcc -print-file-name=libubsan.so)" \
	  ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
	  BSW_ORACLE_LIB=$(ASAN_ORACLE) BSW_SYNTH_LIB=$(ASAN_SYNTH) \
	  python -m pytest tests -q -m "not gpu" -p no:cacheprovider > $(ASAN_DIR)/asan_suite.log 2>&1; rc=$$?; \
	  tail -5 $(ASAN_DIR)/asan_suite.log; exit $$rc
# ThreadSanitizer over the host pipeline's worker thread (Worker, bsw_pool.h): a stand-alone driver, no GPU
TSAN_BIN := $(ASAN_DIR)/worker_driver
$(TSAN_BIN): $(ASAN_DIR)/worker_driver.cpp $(CSRC)/bsw_pool.h
	g++ -fsanitize=thread -fno-omit-frame-pointer -g -O1 -std=c++17 -o $@ $< -lpthread
tsan: $(TSAN_BIN)
	TSAN_OPTIONS=halt_on_error=1 ./$(TSAN_BIN) > $(ASAN_DIR)/tsan.log 2>&1; rc=$$?; cat $(ASAN_DIR)/tsan.log; exit $$rc
.PHONY: asan asan-suite tsan
