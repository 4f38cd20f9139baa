# The morph check (morph_check.cpp: ptsharp_amd/csrc/pt_morph.h's arithmetic, packer, unpacker and argument check driven
# on the host against a plain restatement, and the device layout of pt_update_layout.h), with skin.mk's flags, and once
# more under AddressSanitizer + UndefinedBehaviorSanitizer.
#   make -f morph.mk            _build/morph_check
#   make -f morph.mk asan       _build/morph_check_asan
#   make -f morph.mk run        builds the sanitized program and runs it
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := morph_check.cpp $(CSRC)/pt_morph.h $(CSRC)/pt_update_layout.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h morph.mk
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall $(HIPINC) -I$(CSRC)

morph_check: $(OUT)/morph_check
asan: $(OUT)/morph_check_asan

$(OUT)/morph_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ morph_check.cpp

$(OUT)/morph_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ morph_check.cpp

run: $(OUT)/morph_check_asan
	$(OUT)/morph_check_asan

.PHONY: morph_check asan run
