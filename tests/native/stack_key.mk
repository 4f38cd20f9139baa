# The stack-key checks: stack_key_check.cpp (ptsharp_amd/csrc/pt_stack_key.h, the keyed traversal-stack entries the
# kernels, the scene compile and tools/bvh_quality.cpp share; plain C++, no HIP header, built like bvh8_check) and
# stack_key_scene_check.cpp (the scene compile's choice of the key field on compiled scenes, built like
# scene_compile_check).
#   make -f stack_key.mk                    _build/stack_key_check
#   make -f stack_key.mk scene              _build/stack_key_scene_check
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes

stack_key_check: $(OUT)/stack_key_check
scene: $(OUT)/stack_key_scene_check

$(OUT)/stack_key_check: stack_key_check.cpp $(CSRC)/pt_stack_key.h stack_key.mk
	@mkdir -p $(OUT)
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fno-fast-math -Wall -o $@ stack_key_check.cpp

$(OUT)/stack_key_scene_check: stack_key_scene_check.cpp scene_fixture.h $(CSRC)/pt_stack_key.h $(CSRC)/pt_scene_compile.cpp \
                              $(CSRC)/pt_scene_compile.h $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp \
                              $(CSRC)/pt_bvh.h ../../include/ptsharp_hip.h stack_key.mk
	@mkdir -p $(OUT)
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC) -o $@ stack_key_scene_check.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp

.PHONY: stack_key_check scene
