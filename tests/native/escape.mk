# Where the dropping shade runs: escape_plan_check.cpp (pt::choose_kernels' WfChoice::escape_drop_depths,
# ptsharp_amd/csrc/pt_pass_plan.cpp; plain C++, no HIP header, built like pass_plan_check), and once more under
# AddressSanitizer + UndefinedBehaviorSanitizer.
#   make -f escape.mk           _build/escape_plan_check
#   make -f escape.mk asan      _build/escape_plan_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
DEPS := escape_plan_check.cpp $(CSRC)/pt_pass_plan.cpp $(CSRC)/pt_pass_plan.h ../../include/ptsharp_hip.h escape.mk
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall

escape_plan_check: $(OUT)/escape_plan_check
asan: $(OUT)/escape_plan_check_asan

$(OUT)/escape_plan_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ escape_plan_check.cpp $(CSRC)/pt_pass_plan.cpp

$(OUT)/escape_plan_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ escape_plan_check.cpp $(CSRC)/pt_pass_plan.cpp

.PHONY: escape_plan_check asan
