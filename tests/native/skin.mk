# The skin check (skin_check.cpp: ptsharp_amd/csrc/pt_skin.h driven on the host against a plain restatement of the
# blend of Matrix.MulPosition / MulDirection), with pose.mk's flags, and once more under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f skin.mk            _build/skin_check
#   make -f skin.mk asan       _build/skin_check_asan
#   make -f skin.mk run        builds the sanitized program and runs it
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
DEPS := skin_check.cpp $(CSRC)/pt_skin.h $(CSRC)/pt_pose.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h skin.mk
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall -Wno-unknown-pragmas -I$(CSRC)

skin_check: $(OUT)/skin_check
asan: $(OUT)/skin_check_asan

$(OUT)/skin_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ skin_check.cpp

$(OUT)/skin_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ skin_check.cpp

run: $(OUT)/skin_check_asan
	$(OUT)/skin_check_asan

.PHONY: skin_check asan run
