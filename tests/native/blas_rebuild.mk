# The BLAS rebuild check (blas_rebuild_check.cpp: ptsharp_amd/csrc/pt_blas_rebuild.h driven on the host against the
# scene compile), with blas_check's flags, and once more as a stand-alone program under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f blas_rebuild.mk            _build/blas_rebuild_check
#   make -f blas_rebuild.mk asan       _build/blas_rebuild_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := blas_rebuild_check.cpp scene_fixture.h $(CSRC)/pt_update_layout.h $(CSRC)/pt_blas_rebuild.h $(CSRC)/pt_rebuild.h $(CSRC)/pt_blas_refit.h \
        $(CSRC)/pt_shape_refit.h $(CSRC)/pt_refit.h $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_scene_compile.h $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h \
        $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp $(CSRC)/pt_bvh.h ../../include/ptsharp_hip.h blas_rebuild.mk
SRC := blas_rebuild_check.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC)

blas_rebuild_check: $(OUT)/blas_rebuild_check
asan: $(OUT)/blas_rebuild_check_asan

$(OUT)/blas_rebuild_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ $(SRC)

$(OUT)/blas_rebuild_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $(SRC)

.PHONY: blas_rebuild_check asan
