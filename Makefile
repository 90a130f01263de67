# Builds the in-tree C-ABI library dpdk_dc_sand_amd/libbf.so for gfx950 (MI355X) and the C oracle helpers.
# `python -c "import __graft_entry__ as g; g.build()"` drives this.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CSRC     := dpdk_dc_sand_amd/csrc
LIB      := dpdk_dc_sand_amd/libbf.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -munsafe-fp-atomics
SRCS     := $(CSRC)/bf_runtime.cpp $(CSRC)/bf_coeff.hip $(CSRC)/bf_reorder.hip $(CSRC)/bf_beamform.hip \
            $(CSRC)/bf_fused.hip $(CSRC)/bf_wide.hip $(CSRC)/bf_wide_i8.hip $(CSRC)/bf_q14table.hip $(CSRC)/bf_requant.hip \
            $(CSRC)/bf_study.hip $(CSRC)/bf_incoherent.hip $(CSRC)/bf_detect.hip $(CSRC)/bf_vstats.hip \
            $(CSRC)/bf_correlate.hip $(CSRC)/bf_beam_streams.hip $(CSRC)/bf_dedisperse.hip $(CSRC)/bf_pulse_search.hip \
            $(CSRC)/bf_fold.hip $(CSRC)/bf_pipeline.cpp $(CSRC)/bf_comm.cpp $(CSRC)/bf_fused_plan.cpp
OBJS     := $(patsubst $(CSRC)/%,build/%.o,$(SRCS))
HDRS     := $(wildcard $(CSRC)/*.hpp) include/bf.h

.PHONY: all clean cabi stream dedisperse-naive fold-naive
all: $(LIB) cabi

# bench.py's stream ceiling (the box's best plain stream over a kernel's byte mix): a small measurement library of its
# own, never linked into the product.
STREAM_LIB := build/libbf_stream.so
stream: $(STREAM_LIB)
$(STREAM_LIB): tools/stream_ceiling.hip tools/stream_kernels.hpp
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/bench_ops.py --dedisperse: the one-thread-per-output dedispersion the tiled kernel is measured against; a
# measurement library of its own, never linked into the product.
NAIVE_LIB := build/libbf_dedisperse_naive.so
dedisperse-naive: $(NAIVE_LIB)
$(NAIVE_LIB): tools/dedisperse_naive.hip
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/bench_ops.py --fold: the one-thread-per-(fold, plane, channel) fold the product kernel is measured against; a
# measurement library of its own, never linked into the product.
FOLD_NAIVE_LIB := build/libbf_fold_naive.so
fold-naive: $(FOLD_NAIVE_LIB)
$(FOLD_NAIVE_LIB): tools/fold_naive.hip
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# C callers of the ABI (tests/test_c_abi.py): the harness-order smoke and INTEGRATION.md's streaming example,
# compiled from the markdown block itself.  Plain C against include/bf.h, linked to the in-tree libbf.so.
CC       ?= gcc
CABI     := build/bf_smoke build/bf_stream_doc
cabi: $(CABI)
build/stream_snippet.inc: INTEGRATION.md
	@mkdir -p build
	awk '/<!-- snippet: stream -->/{f=1; next} f && /^```c/{p=1; next} p && /^```/{exit} p' $< > $@
	@test -s $@ || { echo "no stream snippet in INTEGRATION.md"; rm -f $@; exit 1; }
build/bf_smoke: tests/c/bf_smoke.c include/bf.h $(LIB)
	@mkdir -p build
	$(CC) -std=c11 -O2 -Wall -Iinclude $< -o $@ -L$(dir $(LIB)) -lbf -lm -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'
build/bf_stream_doc: tests/c/bf_stream_doc.c build/stream_snippet.inc include/bf.h $(LIB)
	@mkdir -p build
	$(CC) -std=c11 -O2 -Wall -Iinclude -Ibuild $< -o $@ -L$(dir $(LIB)) -lbf -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl

clean:
	rm -rf build $(LIB)
