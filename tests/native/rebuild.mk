# The rebuild check (rebuild_check.cpp: ptsharp_amd/csrc/pt_rebuild.h and pt_refit.h driven on the host against the scene
# compile), with refit_check's flags, and once more under AddressSanitizer + UndefinedBehaviorSanitizer.
#   make -f rebuild.mk            _build/rebuild_check
#   make -f rebuild.mk asan       _build/rebuild_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := rebuild_check.cpp scene_fixture.h layout_parts.h $(CSRC)/pt_update_layout.h $(CSRC)/pt_rebuild.h $(CSRC)/pt_refit.h $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_scene_compile.h \
        $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp $(CSRC)/pt_bvh.h ../../include/ptsharp_hip.h rebuild.mk
SRC := rebuild_check.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC)

rebuild_check: $(OUT)/rebuild_check
asan: $(OUT)/rebuild_check_asan

$(OUT)/rebuild_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ $(SRC)

$(OUT)/rebuild_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $(SRC)

.PHONY: rebuild_check asan
