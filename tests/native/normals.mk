# The normals check (normals_check.cpp: ptsharp_amd/csrc/pt_normals.h driven on the host in the kernels' order, against
# pt_obj.cpp's face normal and pt_mesh_smooth_normals), with refit.mk's flags, and once more under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f normals.mk            _build/normals_check
#   make -f normals.mk asan       _build/normals_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := normals_check.cpp scene_fixture.h $(CSRC)/pt_normals.h $(CSRC)/pt_obj.cpp $(CSRC)/pt_refit.h $(CSRC)/pt_scene_compile.cpp \
        $(CSRC)/pt_scene_compile.h $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp $(CSRC)/pt_bvh.h \
        ../../include/ptsharp_hip.h normals.mk
SRC := normals_check.cpp $(CSRC)/pt_obj.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC)

normals_check: $(OUT)/normals_check
asan: $(OUT)/normals_check_asan

$(OUT)/normals_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ $(SRC)

$(OUT)/normals_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $(SRC)

.PHONY: normals_check asan
