# The look-update check (look_check.cpp: the factored light and flag derivation of ptsharp_amd/csrc/pt_scene_compile.h
# against fresh compiles of the edited scenes, and ptsharp_amd/csrc/pt_texture.h's decode driven on the host in the
# kernel's lane order), with shapes.mk's flags, and once more as a stand-alone program under AddressSanitizer +
# UndefinedBehaviorSanitizer.
#   make -f look.mk            _build/look_check
#   make -f look.mk asan       _build/look_check_asan
#   make -f look.mk run        builds the sanitized program and runs it
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := look_check.cpp scene_fixture.h $(CSRC)/pt_texture.h $(CSRC)/pt_shape_refit.h $(CSRC)/pt_refit.h $(CSRC)/pt_scene_compile.cpp \
        $(CSRC)/pt_scene_compile.h $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h $(CSRC)/pt_volume_update.h $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp \
        $(CSRC)/pt_bvh.h ../../include/ptsharp_hip.h look.mk
SRC := look_check.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC)

look_check: $(OUT)/look_check
asan: $(OUT)/look_check_asan

$(OUT)/look_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ $(SRC)

$(OUT)/look_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $(SRC)

run: $(OUT)/look_check_asan
	$(OUT)/look_check_asan

.PHONY: look_check asan run
