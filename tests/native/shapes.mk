# The shape refit check (shapes_check.cpp: ptsharp_amd/csrc/pt_shape_refit.h driven on the host against the scene
# compile), with scene_compile_check's flags, and once more under AddressSanitizer + UndefinedBehaviorSanitizer.
#   make -f shapes.mk            _build/shapes_check
#   make -f shapes.mk asan       _build/shapes_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := shapes_check.cpp scene_fixture.h layout_parts.h $(CSRC)/pt_update_layout.h $(CSRC)/pt_rebuild.h $(CSRC)/pt_shape_refit.h $(CSRC)/pt_refit.h $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_scene_compile.h \
        $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp $(CSRC)/pt_bvh.h ../../include/ptsharp_hip.h shapes.mk
SRC := shapes_check.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC)

shapes_check: $(OUT)/shapes_check
asan: $(OUT)/shapes_check_asan

$(OUT)/shapes_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ $(SRC)

$(OUT)/shapes_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $(SRC)

.PHONY: shapes_check asan
