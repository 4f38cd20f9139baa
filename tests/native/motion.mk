# The motion check (motion_check.cpp: ptsharp_amd/csrc/pt_motion.h's reprojection and temporal merge driven on the host;
# tests/test_motion_host.py compares what it writes with tests/motion_ref.py), and once more under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f motion.mk            _build/motion_check
#   make -f motion.mk asan       _build/motion_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
DEPS := motion_check.cpp $(CSRC)/pt_motion.h motion.mk
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall -Wno-unknown-pragmas -I$(CSRC)

motion_check: $(OUT)/motion_check
asan: $(OUT)/motion_check_asan

$(OUT)/motion_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ motion_check.cpp

$(OUT)/motion_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ motion_check.cpp

.PHONY: motion_check asan
