# Build the HIP engine in-tree (the .so travels to the GPU box with the snapshot).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := noisyquantumsimulator_amd
SO := $(PKG)/libryd_engine.so
SRC := $(PKG)/csrc/ryd_engine.hip
# the CU-balanced sym16 kernels: a translation unit of their own (it includes $(SRC) up to
# ryd_sym16.inc), because kernel-argument preloading is an option of a whole unit -- their first
# 8 arguments, 14 dwords, arrive in SGPRs -- and every other kernel keeps its code
BAL_SRC := $(PKG)/csrc/ryd_sym16_bal.hip
BAL_FLAGS := -mllvm -amdgpu-kernarg-preload-count=8
OBJDIR ?= build/obj
CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function \
            -ffp-contract=fast -munsafe-fp-atomics
HIPFLAGS := $(CXXFLAGS) -shared
DEPS := $(SRC) $(wildcard $(PKG)/csrc/*.inc) include/ryd_engine.h

all: $(SO)

$(OBJDIR)/ryd_engine.o: $(DEPS)
	mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) $(EXTRA) -c -o $@ $(SRC)

$(OBJDIR)/ryd_sym16_bal.o: $(BAL_SRC) $(DEPS)
	mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) $(EXTRA) $(BAL_FLAGS) -c -o $@ $(BAL_SRC)

$(SO): $(OBJDIR)/ryd_engine.o $(OBJDIR)/ryd_sym16_bal.o
	$(HIPCC) $(HIPFLAGS) -o $@ $^ -ldl

resource-usage: $(SRC) $(BAL_SRC)
	( $(HIPCC) $(CXXFLAGS) -Rpass-analysis=kernel-resource-usage -c -o /tmp/ryd_ru.o $(SRC) 2>&1 ; \
	  $(HIPCC) $(CXXFLAGS) $(BAL_FLAGS) -Rpass-analysis=kernel-resource-usage -c -o /tmp/ryd_ru_bal.o $(BAL_SRC) 2>&1 ) | \
	  grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs:" 

ASM ?= /tmp/ryd_engine.s

# both translation units' device code in one file, the balanced kernels' last
asm: $(SRC) $(BAL_SRC)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC --cuda-device-only -S -o $(ASM) $(SRC)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC $(BAL_FLAGS) --cuda-device-only -S -o $(ASM).bal $(BAL_SRC)
	cat $(ASM).bal >> $(ASM) && rm -f $(ASM).bal

# the inline-asm DPP groups: no VALU write within 2 wait states of a DPP read
check-dpp: asm
	python3 tools/check_dpp_hazards.py $(ASM)

# the gfx950 code of another build (BASE=<its libryd_engine.so>) against this one, kernel by
# kernel: identical disassembly or not, registers / scratch / LDS, instruction-class histograms
kernel-diff: $(SO)
	python3 tools/kernel_diff.py $(BASE) $(SO)

# the refusals of the host-form schedule entry points under AddressSanitizer and UBSan: host code
# only is instrumented, the program is stand-alone and needs no GPU
HOST_REFUSALS ?= build/ryd_host_refusals

host-refusals: $(SRC) $(BAL_SRC) tools/host_refusals.cpp
	mkdir -p $(dir $(HOST_REFUSALS))
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -Wall -Wno-unused-function -ffp-contract=fast \
	  -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined -o $(HOST_REFUSALS) $(SRC) $(BAL_SRC) \
	  tools/host_refusals.cpp -ldl
	$(HOST_REFUSALS)

clean:
	rm -f $(SO) $(OBJDIR)/ryd_engine.o $(OBJDIR)/ryd_sym16_bal.o

.PHONY: all clean resource-usage asm check-dpp kernel-diff host-refusals
