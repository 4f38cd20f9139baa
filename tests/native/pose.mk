# The pose check (pose_check.cpp: ptsharp_amd/csrc/pt_pose.h driven on the host against a plain restatement of
# Matrix.MulPosition / MulDirection), with refit.mk's flags, and once more under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f pose.mk            _build/pose_check
#   make -f pose.mk asan       _build/pose_check_asan
#   make -f pose.mk run        builds the sanitized program and runs it
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
DEPS := pose_check.cpp $(CSRC)/pt_pose.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h pose.mk
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall -Wno-unknown-pragmas -I$(CSRC)

pose_check: $(OUT)/pose_check
asan: $(OUT)/pose_check_asan

$(OUT)/pose_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ pose_check.cpp

$(OUT)/pose_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ pose_check.cpp

run: $(OUT)/pose_check_asan
	$(OUT)/pose_check_asan

.PHONY: pose_check asan run
