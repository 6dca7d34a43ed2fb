# Builds the gfx950 engine (libslacken_amd.so) in-tree, and the CPU oracle used by the tests.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
WPS ?= 0
LWPS ?= 0
LLW ?= 4
EXTRA ?=
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -DSLK_WPS=$(WPS) -DSLK_LANE_WPS=$(LWPS) -DSLK_LANE_LW=$(LLW) $(EXTRA)
CSRC := slacken_amd/csrc
LIB := slacken_amd/lib/libslacken_amd.so

CLI := slacken_amd/bin/slacken-amd

GATHER := slacken_amd/lib/libslk_gather.so

STREAM_SUM := slacken_amd/lib/libslk_stream_sum.so

all: $(LIB) $(CLI) $(GATHER) $(STREAM_SUM) oracle

# measurement helper of bench.py (the part's random-request rate, measured in the bench run): not linked or loaded by the product
$(GATHER): tools/gather_rate.hip
	@mkdir -p slacken_amd/lib
	$(HIPCC) -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -shared -o $@ tools/gather_rate.hip

# measurement helper of tools/bench_taxon_counts.py (a coalesced read-and-sum, the yardstick of the taxon count): not product either
$(STREAM_SUM): tools/stream_sum.hip
	@mkdir -p slacken_amd/lib
	$(HIPCC) -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -shared -o $@ tools/stream_sum.hip

HIPSRC := $(addprefix $(CSRC)/,kernels.hip fused.hip lane.hip build.hip shard.hip wide.hip capi.hip index.hip stream.hip classify.hip shardstep.hip hostcalls.hip shardset.hip bracken.hip migration.hip taxstats.hip respace.hip merge.hip export.hip coverage.hip support.hip textparse.hip readform.hip pipe.hip mask.hip compare.hip)

$(LIB): $(HIPSRC) $(CSRC)/tablebuild.h $(CSRC)/tablewalk.h $(CSRC)/engine.h $(CSRC)/resolve.h $(CSRC)/layouts.h $(CSRC)/laneplan.h $(CSRC)/hostside.h $(CSRC)/pairmap.h $(CSRC)/chunkscan.h $(CSRC)/wavetools.h $(CSRC)/chunkcut.h $(CSRC)/pieces.h $(CSRC)/textlines.h slacken_amd/host/pack.hpp include/slacken_amd.h
	@mkdir -p slacken_amd/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(HIPSRC) -ldl

# Parquet input of the CLI: the Arrow C++ libraries inside the pyarrow wheel, if there is one (no Arrow dev package here)
PYARROW_DIR := $(shell python3 -c "import pyarrow, os; print(os.path.dirname(pyarrow.__file__))" 2>/dev/null)
ifneq ($(wildcard $(PYARROW_DIR)/libparquet.so.*),)
PQ_LIB := $(notdir $(firstword $(sort $(wildcard $(PYARROW_DIR)/libparquet.so.[0-9]*))))
AR_LIB := $(notdir $(firstword $(sort $(wildcard $(PYARROW_DIR)/libarrow.so.[0-9]*))))
PQ_CXXFLAGS := -DSLK_HAVE_PARQUET -I$(PYARROW_DIR)/include
PQ_LDFLAGS := -L$(PYARROW_DIR) -l:$(PQ_LIB) -l:$(AR_LIB) -Wl,-rpath,$(PYARROW_DIR)
endif

slacken_amd/bin/parquet_source.o: slacken_amd/host/parquet_source.cpp slacken_amd/host/parquet_source.hpp
	@mkdir -p slacken_amd/bin
	g++ -O2 -std=c++20 -Wall $(PQ_CXXFLAGS) -c -o $@ slacken_amd/host/parquet_source.cpp

slacken_amd/bin/parquet_sink.o: slacken_amd/host/parquet_sink.cpp slacken_amd/host/library_writer.hpp slacken_amd/host/parquet_source.hpp
	@mkdir -p slacken_amd/bin
	g++ -O2 -std=c++20 -Wall $(PQ_CXXFLAGS) -c -o $@ slacken_amd/host/parquet_sink.cpp

$(CLI): slacken_amd/bin/parquet_source.o slacken_amd/bin/parquet_sink.o slacken_amd/host/slacken_cli.cpp $(wildcard slacken_amd/host/*.hpp) include/slacken_amd.h $(LIB)
	@mkdir -p slacken_amd/bin
	g++ -O2 -std=c++17 -Wall -o $@ slacken_amd/host/slacken_cli.cpp slacken_amd/bin/parquet_source.o slacken_amd/bin/parquet_sink.o $(PQ_LDFLAGS) -Lslacken_amd/lib -lslacken_amd -lz -ldl -lpthread -Wl,-rpath,'$$ORIGIN/../lib'

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(GATHER) $(STREAM_SUM)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
