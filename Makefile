# Build of the MI355X (gfx950) admission engine. `python -c "import __graft_entry__ as g; g.build()"`
# runs this; hipcc cross-compiles for gfx950 without a GPU.
#   policy-server_amd/libkwgpu.so    product: HIP kernels + host engine + C ABI (include/kwgpu.h)
#   policy-server_amd/libkwsynth.so  bench/test workload generator
#   policy-server_amd/kwhost         HTTP front (/validate, /audit, /validate_raw) over libkwgpu.so
#   policy-server_amd/kwload         closed-loop HTTP load generator for kwhost (serving measurement)
#   oracle/build/libkworacle.so      CPU restatement (test infrastructure only)
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
CC ?= gcc
ARCH ?= gfx950
PKG := policy-server_amd
SRC := $(PKG)/csrc
OBJ := $(PKG)/build
HIPDEF := -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
CXXFLAGS := -O3 -std=c++17 -fPIC -Wall -Wextra $(HIPDEF)
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -munsafe-fp-atomics $(HIPEXTRA)

HOST_SRCS := json yaml automaton expr env flatten service slotplan metrics knobs pools plan pass upload bulk bulkout packed lastpass summary outcomes digest members messages responses patches capi
HOST_OBJS := $(addprefix $(OBJ)/,$(addsuffix .o,$(HOST_SRCS)))
# the device objects: the hot path (kernels.hip), the reports over its verdict words (reports.hip)
# and the wide path's combine kernel with the group programs' VM (groups.hip)
DEV_SRCS := kernels reports groups
DEV_OBJS := $(addprefix $(OBJ)/,$(addsuffix .o,$(DEV_SRCS)))
VOBJ = $(PKG)/variants/obj-$(NAME)

all: $(PKG)/libkwgpu.so $(PKG)/libkwsynth.so $(PKG)/kwhost $(PKG)/kwload oracle/build/libkworacle.so scripts/lds_calib scripts/lds_occ scripts/fmt_bench

# kwhost's host stages (flatten, response JSON) timed without a GPU
scripts/fmt_bench: scripts/fmt_bench.cpp include/kwgpu.h $(PKG)/libkwgpu.so $(PKG)/libkwsynth.so
	$(CXX) -O2 -std=c++17 $< -o $@ -L$(PKG) -lkwgpu -lkwsynth -Wl,-rpath,'$$ORIGIN/../$(PKG)'

# LDS counter calibration micro-kernels (scripts/lds_calib.sh runs them under rocprofv3 --pmc)
scripts/lds_calib: scripts/lds_calib.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -o $@ $<

# LDS residency probe: workgroups a CU holds per dynamic LDS size (profiles/r05_lds_residency.txt)
scripts/lds_occ: scripts/lds_occ.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -o $@ $<

# every object depends on the headers it includes, as the compiler lists them (build/*.d). An
# object left by a build that wrote no list (this Makefile before DEV_SRCS) has none: run
# `make clean` once over such a build/, or header edits will not reach those objects.
$(OBJ)/%.o: $(SRC)/%.cpp
	@mkdir -p $(OBJ)
	$(CXX) $(CXXFLAGS) -MMD -MP -c $< -o $@

$(DEV_OBJS): $(OBJ)/%.o: $(SRC)/%.hip
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

-include $(HOST_OBJS:.o=.d) $(DEV_OBJS:.o=.d)

$(PKG)/libkwgpu.so: $(HOST_OBJS) $(DEV_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(PKG)/kwhost: $(SRC)/kwhost.cpp include/kwgpu.h $(PKG)/libkwgpu.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ $< -L$(PKG) -lkwgpu -Wl,-rpath,'$$ORIGIN' -lpthread

$(PKG)/kwload: $(SRC)/kwload.cpp $(PKG)/libkwsynth.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ $< -L$(PKG) -lkwsynth -Wl,-rpath,'$$ORIGIN' -lpthread

$(PKG)/libkwsynth.so: $(SRC)/synth.cpp include/kwgpu.h
	$(CXX) -O3 -std=c++17 -fPIC -shared -Wall -o $@ $<

oracle/build/libkworacle.so: oracle/kworacle.c oracle/kwregex.c oracle/kworacle.h oracle/unicode_data.h include/kwgpu.h
	@mkdir -p oracle/build
	$(CC) -O2 -std=c11 -fPIC -shared -Wall -Wextra -o $@ oracle/kworacle.c oracle/kwregex.c -lpthread

# A/B variant of the library with extra kernel flags: make variant NAME=x VFLAGS="-DKW_PREFETCH=0"
# -> policy-server_amd/variants/x.so (KWGPU_LIB selects it; scripts/ab.sh benches every variant);
# KSRC=<file in csrc/> builds another kernels source in place of kernels.hip (e.g. the previous commit's)
variant: $(HOST_OBJS)
	@mkdir -p $(VOBJ)
	for f in $(DEV_SRCS); do src=$(SRC)/$$f.hip; [ $$f = kernels ] && src=$(or $(KSRC),$(SRC)/kernels.hip); \
	  $(HIPCC) $(HIPFLAGS) $(VFLAGS) -c $$src -o $(VOBJ)/$$f.o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(PKG)/variants/$(NAME).so $(HOST_OBJS) $(addprefix $(VOBJ)/,$(addsuffix .o,$(DEV_SRCS)))

# A/B variant built entirely (host engine + kernels) from another source directory next to csrc/,
# e.g. a snapshot of an earlier commit: make variant-full NAME=x VSRC=policy-server_amd/csrc_x
# (of the device sources, those the snapshot has: an earlier commit may hold fewer)
variant-full:
	@mkdir -p $(VOBJ)
	for f in $(HOST_SRCS); do $(CXX) $(CXXFLAGS) $(VFLAGS) -c $(VSRC)/$$f.cpp -o $(VOBJ)/$$f.o || exit 1; done
	objs=; for f in $(DEV_SRCS); do [ -f $(VSRC)/$$f.hip ] || continue; \
	  $(HIPCC) $(HIPFLAGS) $(VFLAGS) -c $(VSRC)/$$f.hip -o $(VOBJ)/$$f.o || exit 1; objs="$$objs $(VOBJ)/$$f.o"; done; \
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(PKG)/variants/$(NAME).so $(addprefix $(VOBJ)/,$(addsuffix .o,$(HOST_SRCS))) $$objs

# kernel resource usage (VGPR/SGPR/LDS/occupancy) report
resources: $(addprefix $(SRC)/,$(addsuffix .hip,$(DEV_SRCS)))
	for f in $^; do $(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $$f -o /dev/null || exit 1; done

clean:
	rm -rf $(OBJ) $(PKG)/*.so $(PKG)/kwhost $(PKG)/kwload oracle/build

.PHONY: all clean resources variant variant-full
