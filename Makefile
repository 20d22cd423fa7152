# Build everything in-tree (the built .so files travel to the GPU box with the snapshot).
#   make            -> product: xalm_amd/lib/libxalm_hip.so, libxalm_host.so, xalm_amd/bin/xalm
#                      test infrastructure: oracle/lib/liboracle.so
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
CC ?= gcc
ARCH ?= gfx950

HIPFLAGS := -O3 --offload-arch=$(ARCH) -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result $(HIPFLAGS_EXTRA)
HOSTFLAGS := -O2 -std=c++17 -fPIC -Wall -Wextra

LIB := xalm_amd/lib
BIN := xalm_amd/bin
HIP_UNITS := xalm_hip launch decode prefill prefill_blas upload ops
HOST_SRC := $(wildcard xalm_amd/host/*.cpp)
HOST_HDR := $(wildcard xalm_amd/host/*.h) include/xalm_hip.h include/xalm_host.h

.PHONY: all product oracle clean
all: product oracle
ifneq ($(HOST_SRC),)
product: $(LIB)/libxalm_hip.so $(LIB)/libxalm_host.so $(BIN)/xalm
else
product: $(LIB)/libxalm_hip.so
endif
oracle:
	$(MAKE) -C oracle

# one object per host unit; the fused attention + Wo kernel (dt_launch.hip) once per Wo dtype.
# Every object depends on the headers it includes (-MMD).
OBJ := xalm_amd/build
PK_DTS := 1 2 3 6 7 9
HIP_OBJS := $(patsubst %,$(OBJ)/%.o,$(HIP_UNITS)) $(patsubst %,$(OBJ)/dt_launch_dt%.o,$(PK_DTS))
$(OBJ)/%.o: xalm_amd/csrc/%.hip
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c -o $@ $<
$(OBJ)/dt_launch_dt%.o: xalm_amd/csrc/dt_launch.hip
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -DPK_DT=$* -c -o $@ $<
# the regex compiler and the host mask: plain C++, no HIP
$(OBJ)/constraint.o: xalm_amd/csrc/constraint.cpp
	@mkdir -p $(OBJ)
	$(CXX) $(HOSTFLAGS) -MMD -MP -c -o $@ $<
# the host top-N log-probabilities and their argument checks: plain C++ likewise
$(OBJ)/top_logprobs.o: xalm_amd/csrc/top_logprobs.cpp
	@mkdir -p $(OBJ)
	$(CXX) $(HOSTFLAGS) -MMD -MP -c -o $@ $<
# the host mirror of the adaptive truncation: plain C++, every f32 operation rounded on its own
$(OBJ)/truncate.o: xalm_amd/csrc/truncate.cpp
	@mkdir -p $(OBJ)
	$(CXX) $(HOSTFLAGS) -ffp-contract=off -MMD -MP -c -o $@ $<
# the host mirror of DRY, the n-gram ban and XTC: plain C++ likewise
$(OBJ)/seq_host.o: xalm_amd/csrc/seq_host.cpp
	@mkdir -p $(OBJ)
	$(CXX) $(HOSTFLAGS) -ffp-contract=off -MMD -MP -c -o $@ $<
# the host definition of the fp8 KV ring's element: plain C++, integer arithmetic
$(OBJ)/kv8.o: xalm_amd/csrc/kv8.cpp
	@mkdir -p $(OBJ)
	$(CXX) $(HOSTFLAGS) -MMD -MP -c -o $@ $<
HIP_OBJS += $(OBJ)/constraint.o $(OBJ)/top_logprobs.o $(OBJ)/truncate.o $(OBJ)/seq_host.o $(OBJ)/kv8.o
$(LIB)/libxalm_hip.so: $(HIP_OBJS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $^
$(HIP_OBJS:.o=.d): ;
-include $(HIP_OBJS:.o=.d)

HOST_LIB_SRC := $(filter-out xalm_amd/host/main.cpp,$(HOST_SRC))
$(LIB)/libxalm_host.so: $(HOST_LIB_SRC) $(HOST_HDR) $(LIB)/libxalm_hip.so
	$(CXX) $(HOSTFLAGS) -fopenmp -shared -o $@ $(HOST_LIB_SRC) -L$(LIB) -lxalm_hip -Wl,-rpath,'$$ORIGIN'

$(BIN)/xalm: xalm_amd/host/main.cpp $(LIB)/libxalm_host.so
	@mkdir -p $(BIN)
	$(CXX) $(HOSTFLAGS) -o $@ xalm_amd/host/main.cpp -L$(LIB) -lxalm_host -lxalm_hip -Wl,-rpath,'$$ORIGIN/../lib'

clean:
	rm -rf $(LIB) $(BIN) $(OBJ)
	$(MAKE) -C oracle clean
