# Build for MI355X (gfx950).  `make` builds the product library and the CPU oracle.
#   lumo_amd/liblumo_amd.so   product: host scene builder (C++) + HIP wavefront kernels + C ABI
#   oracle/_build/liblumo_oracle.so   test infrastructure (CPU restatement), never linked by the product
# Strict IEEE f64: no FMA contraction anywhere (parity with the scalar restatement).

HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
ARCH     ?= gfx950
JOBS     ?= 8
FPFLAGS  := -ffp-contract=off -fno-fast-math
CXXFLAGS := -O2 -std=c++17 -fPIC $(FPFLAGS) -Wall -Wextra -Wno-unused-parameter
HIPFLAGS := -O3 -std=c++17 -fPIC $(FPFLAGS) --offload-arch=$(ARCH) -Wall -Wno-unused-parameter \
            -munsafe-fp-atomics

HOST_SRC := $(wildcard lumo_amd/csrc/host/*.cpp)
BUILD    ?= build
HOST_OBJ := $(patsubst lumo_amd/csrc/host/%.cpp,build/host/%.o,$(HOST_SRC))
# kernels.hip: the non-traversal kernels, the schedulers and the entry points that launch them;
# ctx.hip (context, options) and upload.hip (scene, camera) are host code only and share ctx.h with
# it.  The traversal kernels are instantiated once per kd stack class (launch.h STACK_CLASSES) in
# their own translation units, so they compile in parallel: inst_pt.hip / inst_bd.hip built with
# -DLUMO_STK=<class>.
STK_CLASSES := 0 4 8 16 24 32 48 64
MAIN_OBJ := $(BUILD)/device/kernels.o $(BUILD)/device/ctx.o $(BUILD)/device/upload.o
DEV_OBJ  := $(MAIN_OBJ) $(foreach k,$(STK_CLASSES),$(BUILD)/device/inst_pt_$(k).o $(BUILD)/device/inst_bd_$(k).o)
CTX_H    := lumo_amd/csrc/device/ctx.h lumo_amd/csrc/host/wbvh.h
DEV_H    := $(filter-out $(CTX_H),$(wildcard lumo_amd/csrc/device/*.h))
COMMON_H := $(wildcard lumo_amd/csrc/common/*.h) include/lumo_amd.h include/lumo_host.h

LIB      ?= lumo_amd/liblumo_amd.so
ORACLE   := oracle/_build/liblumo_oracle.so
ORACLE_G := oracle/_build/liblumo_oracle_glibc.so

all: $(LIB) $(ORACLE) $(ORACLE_G)

build/host/%.o: lumo_amd/csrc/host/%.cpp $(COMMON_H) $(wildcard lumo_amd/csrc/host/*.h)
	@mkdir -p build/host
	$(CXX) $(CXXFLAGS) -c $< -o $@

$(MAIN_OBJ): $(BUILD)/device/%.o: lumo_amd/csrc/device/%.hip $(COMMON_H) $(DEV_H) $(CTX_H)
	@mkdir -p $(BUILD)/device
	$(HIPCC) $(HIPFLAGS) $(DEVFLAGS) -c $< -o $@

$(BUILD)/device/inst_pt_%.o: lumo_amd/csrc/device/inst_pt.hip $(COMMON_H) $(DEV_H)
	@mkdir -p $(BUILD)/device
	$(HIPCC) $(HIPFLAGS) $(DEVFLAGS) -DLUMO_STK=$* -c $< -o $@

$(BUILD)/device/inst_bd_%.o: lumo_amd/csrc/device/inst_bd.hip $(COMMON_H) $(DEV_H)
	@mkdir -p $(BUILD)/device
	$(HIPCC) $(HIPFLAGS) $(DEVFLAGS) -DLUMO_STK=$* -c $< -o $@

$(LIB): $(HOST_OBJ) $(DEV_OBJ)
	$(HIPCC) -shared --offload-arch=$(ARCH) -o $@ $^ -lpthread -lz

$(ORACLE): oracle/src/oracle.cpp oracle/oracle.h $(COMMON_H)
	@mkdir -p oracle/_build
	$(CXX) $(CXXFLAGS) -O2 -shared -o $@ oracle/src/oracle.cpp -lpthread

$(ORACLE_G): oracle/src/oracle.cpp oracle/oracle.h $(COMMON_H)
	@mkdir -p oracle/_build
	$(CXX) $(CXXFLAGS) -O2 -DLUMO_ORACLE_GLIBC -shared -o $@ oracle/src/oracle.cpp -lpthread

# Sanitizer build (CPU only): the host library sources and the oracle under ASan + UBSan, driven by
# tools/sanitize/main.cpp (scene builds, both integrators, textures, hostile PNG / HDR / OBJ input).
SAN_FLAGS := -O1 -g -std=c++17 $(FPFLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all \
             -fno-omit-frame-pointer -Wall -Wno-unused-parameter
build/sanitize/lumo_sanitize: tools/sanitize/main.cpp $(HOST_SRC) oracle/src/oracle.cpp oracle/oracle.h $(COMMON_H) \
                              $(wildcard lumo_amd/csrc/host/*.h)
	@mkdir -p build/sanitize
	$(CXX) $(SAN_FLAGS) -o $@ tools/sanitize/main.cpp $(HOST_SRC) oracle/src/oracle.cpp -lpthread -lz

sanitize: build/sanitize/lumo_sanitize
	ASAN_OPTIONS=halt_on_error=1:detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	    ./build/sanitize/lumo_sanitize

# A/B builds of the device code (perf experiments, loaded with LUMO_AMD_LIB=<path>):
#   make variant NAME=slab0 DEVFLAGS=-DLUMO_REUSE_SLAB=0   ->  lumo_amd/var/liblumo_amd_slab0.so
variant:
	@mkdir -p lumo_amd/var
	$(MAKE) BUILD=build/var_$(NAME) LIB=lumo_amd/var/liblumo_amd_$(NAME).so DEVFLAGS="$(DEVFLAGS)" lumo_amd/var/liblumo_amd_$(NAME).so


clean:
	rm -rf build $(LIB) oracle/_build lumo_amd/var

.PHONY: all clean variant sanitize
