# Build libminehip.so (gfx950 HIP kernels + C-ABI) and the CPU oracle.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
PKG     := bitcoin-miner_amd
CSRC    := $(PKG)/csrc
LIB     := $(PKG)/minehip/libminehip.so
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-result
SRCS    := $(CSRC)/search_kernels.hip $(CSRC)/minehip.cpp $(CSRC)/batch.cpp $(CSRC)/plan.cpp $(CSRC)/multi.cpp $(CSRC)/message.cpp \
           $(CSRC)/sched.cpp $(CSRC)/server.cpp
HDRS    := $(CSRC)/layout.hpp $(CSRC)/plan.hpp $(CSRC)/host_ctx.hpp $(CSRC)/sha256_gfx950.hpp $(CSRC)/msgcodec.hpp \
           $(CSRC)/sched.hpp $(CSRC)/multi.hpp $(CSRC)/kernel_common.hpp include/minehip.h include/minehip_server.h
LLVM    ?= /opt/rocm/lib/llvm/bin
BUILD   := build
FAST_HDRS := $(CSRC)/kernel_common.hpp $(CSRC)/layout.hpp $(CSRC)/sha256_gfx950.hpp
FAST_S  := $(BUILD)/fast_search.s
FAST_SP := $(BUILD)/fast_search_split.s
FAST_PS := $(BUILD)/fast_search_prio.s
FAST_MIX := $(BUILD)/fast_loop_mix.json
# every ADD3_SPLIT-th v_add3 of each fast kernel as two full-rate adds (csrc/add3_split.py; 0: none)
ADD3_SPLIT ?= 3
FAST_CO := $(BUILD)/fast_search.hsaco
FAST_O  := $(BUILD)/fast_co.o
FASTFLAGS ?=
# the code objects built from fast_search.hip, every one through the same passes: the product's
# (embedded in the library), the coarse-hash test variant (-DMH_HASH_KEEP) and the
# first-hit kernels first_scan<J, MODE> of mh_search_first (-DMH_FIRST; embedded too)
# and the hits kernels hits_scan<J, MODE> of mh_search_hits (-DMH_HITS; embedded too)
# and the batch kernels batch_fast<J, MODE> of mh_search_batch_ex (-DMH_BATCH; embedded
# too) with their coarse-hash test variant (-DMH_BATCH -DMH_HASH_KEEP, the dev build's
# MINEHIP_DEV_BATCH_CODE_OBJECT) and the first-hit batch kernels batch_first<J, MODE> of
# mh_search_first_batch_ex (-DMH_BATCH -DMH_FIRST; embedded too, no test variant) and the
# hits batch kernels batch_hits<J, MODE> of mh_search_hits_batch_ex (-DMH_BATCH -DMH_HITS; likewise)
# and the stopping first-hit kernels stop_scan<J, MODE> of mh_search_first_ex (-DMH_FIRST -DMH_STOP,
# DESIGN.md §3; embedded too, no test variant) and the stopping first-hit batch kernels
# batch_stop<J, MODE> of mh_search_first_batch_stop (-DMH_BATCH -DMH_FIRST -DMH_STOP; likewise) and the
# stopping hits kernels hits_stop<J, MODE> of mh_search_first_hits (-DMH_HITS -DMH_STOP; likewise) and the
# stopping hits batch kernels batch_bound<J, MODE> of mh_search_first_hits_batch (-DMH_BATCH -DMH_HITS
# -DMH_STOP; likewise)
FAST_NAMES := fast_search fast_search_keep fast_first fast_hits fast_batch fast_batch_keep fast_batch_first fast_batch_hits \
              fast_first_stop fast_batch_first_stop fast_hits_stop fast_batch_bound
FASTFLAGS_fast_search_keep := -DMH_HASH_KEEP
FASTFLAGS_fast_first := -DMH_FIRST
FASTFLAGS_fast_hits := -DMH_HITS
FASTFLAGS_fast_batch := -DMH_BATCH
FASTFLAGS_fast_batch_keep := -DMH_BATCH -DMH_HASH_KEEP
FASTFLAGS_fast_batch_first := -DMH_BATCH -DMH_FIRST
FASTFLAGS_fast_batch_hits := -DMH_BATCH -DMH_HITS
FASTFLAGS_fast_first_stop := -DMH_FIRST -DMH_STOP
FASTFLAGS_fast_batch_first_stop := -DMH_BATCH -DMH_FIRST -DMH_STOP
FASTFLAGS_fast_hits_stop := -DMH_HITS -DMH_STOP
FASTFLAGS_fast_batch_bound := -DMH_BATCH -DMH_HITS -DMH_STOP
FIRST_CO := $(BUILD)/fast_first.hsaco
HITS_CO := $(BUILD)/fast_hits.hsaco
BATCH_CO := $(BUILD)/fast_batch.hsaco
BATCH_FIRST_CO := $(BUILD)/fast_batch_first.hsaco
BATCH_HITS_CO := $(BUILD)/fast_batch_hits.hsaco
FIRST_STOP_CO := $(BUILD)/fast_first_stop.hsaco
BATCH_FIRST_STOP_CO := $(BUILD)/fast_batch_first_stop.hsaco
HITS_STOP_CO := $(BUILD)/fast_hits_stop.hsaco
BATCH_BOUND_CO := $(BUILD)/fast_batch_bound.hsaco

LSPLIB  := $(PKG)/minehip/liblsp440.so
APPS    := $(CSRC)/apps
BIN     := $(PKG)/bin
CLIS    := $(BIN)/minehip-search $(BIN)/minehip-miner $(BIN)/minehip-server $(BIN)/minehip-client
RPATH   := -Wl,-rpath,'$$ORIGIN/../minehip'

DEVLIB  := $(BUILD)/dev/libminehip.so

all: $(LIB) $(LSPLIB) $(CLIS) oracle dev $(BUILD)/libclockprobe.so $(BUILD)/libvaluenergy.so $(FAST_MIX) $(BUILD)/fast_search_nomarker.hsaco \
     $(BUILD)/fast_search_keep.hsaco $(BUILD)/fast_batch_keep.hsaco

# LSP endpoint (host only, wire compatible with the reference's Go lsp package)
$(LSPLIB): $(CSRC)/lsp/lsp.cpp include/lsp440.h
	g++ -O2 -std=c++17 -Wall -Wextra -fPIC -shared -o $@ $(CSRC)/lsp/lsp.cpp -lpthread

$(LIB): $(SRCS) $(HDRS) $(FAST_O)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SRCS) -x none $(FAST_O)

# dev build: the same library plus the experiment / test hooks (MINEHIP_DEV_CODE_OBJECT,
# MINEHIP_DEV_LDS, MINEHIP_TEST_FAIL_WORKER, MINEHIP_TEST_SPAWN_LIMIT, and MINEHIP_DEV_HASH_KEEP=k0,k1: every hash
# cut to its top k0 + k1 bits so that nonces tie, with build/fast_search_keep.hsaco as the fast code object,
# tests/test_gpu_ties.py; MINEHIP_DEV_HASH_XOR=<hex>: every hash XORed with a 64-bit constant before that cut, so
# that a test chooses the winning nonce, with the same code object, tests/test_gpu_probe.py).  Never the package's library: tools and the tests that need a hook load it
# explicitly (MINEHIP_LIB=build/dev/libminehip.so).
dev: $(DEVLIB)
$(DEVLIB): $(SRCS) $(HDRS) $(FAST_O)
	mkdir -p $(BUILD)/dev
	$(HIPCC) $(HIPFLAGS) -DMH_DEV_HOOKS -shared -o $@ $(SRCS) -x none $(FAST_O)

# fast_search<J, MODE>: gfx950 assembly -> add3 split (every third v_add3 as two full-rate adds)
# -> issue-priority pass (s_setprio around half-/full-rate runs) -> code object ->
# embedded in the library (fast_co.S); the per-nonce loops' issued mix -> fast_loop_mix.json (bench)
# ($* is the code object's name, one of FAST_NAMES; the product's files are FAST_S, FAST_SP, FAST_PS, FAST_CO)
$(FAST_NAMES:%=$(BUILD)/%.s): $(BUILD)/%.s: $(CSRC)/fast_search.hip $(FAST_HDRS)
	mkdir -p $(BUILD)
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) $(FASTFLAGS) $(FASTFLAGS_$*) --cuda-device-only -S -o $@ $<
# the split factor is a prerequisite: `make ADD3_SPLIT=k` after a build redoes the split (and the
# loop mix bench.py reads) instead of reusing the old assembly
ADD3_STAMP := $(BUILD)/add3_split.$(ADD3_SPLIT).stamp
$(ADD3_STAMP):
	mkdir -p $(BUILD)
	rm -f $(BUILD)/add3_split.*.stamp
	touch $@
$(FAST_NAMES:%=$(BUILD)/%_split.s): $(BUILD)/%_split.s: $(BUILD)/%.s $(CSRC)/add3_split.py $(ADD3_STAMP)
	python3 $(CSRC)/add3_split.py $(ADD3_SPLIT) $< $@ $(ADD3_LIKE_$*)
# the first-hit, stopping first-hit, hits and batch builds split their per-nonce loops as the product's are split (add3_split.py, like_split.s)
ADD3_LIKE_fast_first := $(FAST_SP)
ADD3_LIKE_fast_hits := $(FAST_SP)
ADD3_LIKE_fast_batch := $(FAST_SP)
ADD3_LIKE_fast_batch_keep := $(FAST_SP)
ADD3_LIKE_fast_batch_first := $(FAST_SP)
ADD3_LIKE_fast_batch_hits := $(FAST_SP)
ADD3_LIKE_fast_first_stop := $(FAST_SP)
ADD3_LIKE_fast_batch_first_stop := $(FAST_SP)
ADD3_LIKE_fast_hits_stop := $(FAST_SP)
ADD3_LIKE_fast_batch_bound := $(FAST_SP)
$(BUILD)/fast_first_split.s $(BUILD)/fast_hits_split.s $(BUILD)/fast_batch_split.s $(BUILD)/fast_batch_keep_split.s \
$(BUILD)/fast_batch_first_split.s $(BUILD)/fast_batch_hits_split.s $(BUILD)/fast_first_stop_split.s \
$(BUILD)/fast_batch_first_stop_split.s $(BUILD)/fast_hits_stop_split.s $(BUILD)/fast_batch_bound_split.s: $(FAST_SP) $(CSRC)/loop_mix.py
$(FAST_NAMES:%=$(BUILD)/%_prio.s): $(BUILD)/%_prio.s: $(BUILD)/%_split.s $(CSRC)/issue_prio.py $(CSRC)/valu_rates.py
	python3 $(CSRC)/issue_prio.py $< $@
$(FAST_MIX): $(FAST_PS) $(CSRC)/loop_mix.py $(CSRC)/valu_rates.py
	python3 $(CSRC)/loop_mix.py $< $@
$(FAST_NAMES:%=$(BUILD)/%.hsaco): $(BUILD)/%.hsaco: $(BUILD)/%_prio.s
	$(LLVM)/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=$(ARCH) -c -o $(BUILD)/$*_prio.o $<
	$(LLVM)/ld.lld -shared -o $@ $(BUILD)/$*_prio.o
# test artefact: the same kernels without the work-queue marker (mh_fast_queue_args), as a code
# object built from older sources would be; the dev build must run it one workgroup per chunk
# (tests/test_gpu_parity.py::test_code_object_without_queue_marker_runs_static)
$(BUILD)/fast_search_nomarker.hsaco: $(FAST_PS)
	grep -v mh_fast_queue_args $< > $(BUILD)/fast_search_nomarker.s
	$(LLVM)/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=$(ARCH) -c -o $(BUILD)/fast_search_nomarker.o $(BUILD)/fast_search_nomarker.s
	$(LLVM)/ld.lld -shared -o $@ $(BUILD)/fast_search_nomarker.o
$(FAST_O): $(CSRC)/fast_co.S $(FAST_CO) $(FIRST_CO) $(HITS_CO) $(BATCH_CO) $(BATCH_FIRST_CO) $(BATCH_HITS_CO) $(FIRST_STOP_CO) \
           $(BATCH_FIRST_STOP_CO) $(HITS_STOP_CO) $(BATCH_BOUND_CO)
	gcc -c -fPIC -Wa,-I,$(BUILD) -o $@ $<

# native C++ callers of the C-ABI (rpath: the library next to the package)
$(BIN)/minehip-search: $(CSRC)/cli.cpp include/minehip.h $(LIB)
	mkdir -p $(BIN)
	g++ -O2 -std=c++17 -Wall -o $@ $(CSRC)/cli.cpp -L$(PKG)/minehip -lminehip $(RPATH)

# miner / server / client processes over LSP (bitcoin/{miner,server,client})
$(BIN)/minehip-%: $(APPS)/%_main.cpp $(APPS)/common.hpp include/minehip.h include/minehip_server.h include/lsp440.h $(LIB) $(LSPLIB)
	mkdir -p $(BIN)
	g++ -O2 -std=c++17 -Wall -Wextra -o $@ $< -L$(PKG)/minehip -lminehip -llsp440 $(RPATH) -lpthread

oracle:
	$(MAKE) -s -C oracle

# in-kernel clock probe (measurement only: bench.py's roofline.kernel_clock)
$(BUILD)/libclockprobe.so: tools/clock_probe.hip
	mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# energy per VALU instruction class at the power limit (measurement only: tools/energy_probe.py)
$(BUILD)/libvaluenergy.so: tools/valu_energy.hip
	mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# disassembly + register report of the kernels (for DESIGN.md / profiling)
asm: $(FAST_PS)
	mkdir -p build
	$(HIPCC) $(HIPFLAGS) --cuda-device-only -S -o build/search_kernels.s $(CSRC)/search_kernels.hip

# VALU issue-rate microbenchmarks, run by tools/gpu_session.sh
probes: build/valu_peak build/valu_ops build/valu_mix build/valu_pair build/valu_bank
build/valu_bank: tools/gen_valu_bank.py
	mkdir -p build
	python3 tools/gen_valu_bank.py build/valu_bank.hip
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -o $@ build/valu_bank.hip
build/valu_pair: tools/gen_valu_pair.py
	mkdir -p build
	python3 tools/gen_valu_pair.py build/valu_pair.hip
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -o $@ build/valu_pair.hip
build/valu_mix: tools/gen_valu_mix.py
	mkdir -p build
	python3 tools/gen_valu_mix.py build/valu_mix.hip
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -o $@ build/valu_mix.hip
build/valu_%: tools/valu_%.hip
	mkdir -p build
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -o $@ $<

clean:
	rm -f $(LIB) $(DEVLIB) $(LSPLIB) $(CLIS) $(FAST_MIX) $(FAST_O) \
	      $(foreach n,$(FAST_NAMES),$(BUILD)/$(n).s $(BUILD)/$(n)_split.s $(BUILD)/$(n)_prio.s $(BUILD)/$(n)_prio.o $(BUILD)/$(n).hsaco) \
	      $(BUILD)/libclockprobe.so $(BUILD)/libvaluenergy.so $(BUILD)/add3_split.*.stamp \
	      $(BUILD)/fast_search_nomarker.*
	$(MAKE) -s -C oracle clean

.PHONY: all oracle asm clean probes dev
