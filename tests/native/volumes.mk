# The volume-update check (volumes_check.cpp: ptsharp_amd/csrc/pt_volume_update.h driven on the host, cell by cell,
# against a plain restatement of the upload's old table loops; the argument check, the light test and the 64-bit
# indices), with pose.mk's flags, and once more as a stand-alone program under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f volumes.mk            _build/volumes_check
#   make -f volumes.mk asan       _build/volumes_check_asan
#   make -f volumes.mk run        builds the sanitized program and runs it
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
DEPS := volumes_check.cpp $(CSRC)/pt_volume_update.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h ../../include/ptsharp_hip.h volumes.mk
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall -Wno-unknown-pragmas -I$(CSRC)

volumes_check: $(OUT)/volumes_check
asan: $(OUT)/volumes_check_asan

$(OUT)/volumes_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ volumes_check.cpp

$(OUT)/volumes_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ volumes_check.cpp

run: $(OUT)/volumes_check_asan
	$(OUT)/volumes_check_asan

.PHONY: volumes_check asan run
