# Build the HIP engine in-tree (the .so travels to the GPU box with the snapshot).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := noisyquantumsimulator_amd
SO := $(PKG)/libryd_engine.so
SRC := $(PKG)/csrc/ryd_engine.hip
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-function \
            -ffp-contract=fast -munsafe-fp-atomics

all: $(SO)

$(SO): $(SRC) $(wildcard $(PKG)/csrc/*.inc) include/ryd_engine.h
	$(HIPCC) $(HIPFLAGS) -o $@ $(SRC) -ldl

resource-usage: $(SRC)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -o /tmp/ryd_ru.so $(SRC) 2>&1 | \
	  grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs:" 

ASM ?= /tmp/ryd_engine.s

asm: $(SRC)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC --cuda-device-only -S -o $(ASM) $(SRC)

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

host-refusals: $(SRC) tools/host_refusals.cpp
	mkdir -p $(dir $(HOST_REFUSALS))
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -Wall -Wno-unused-function -ffp-contract=fast \
	  -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined -o $(HOST_REFUSALS) $(SRC) \
	  tools/host_refusals.cpp -ldl
	$(HOST_REFUSALS)

clean:
	rm -f $(SO)

.PHONY: all clean resource-usage asm check-dpp kernel-diff host-refusals
