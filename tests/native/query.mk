# The query tables check (query_tables_check.cpp: the identity tables of pt_intersect_hits from the scene compile, on the
# host), with rebuild_check's flags, and once more under AddressSanitizer + UndefinedBehaviorSanitizer.
#   make -f query.mk            _build/query_tables_check
#   make -f query.mk asan       _build/query_tables_check_asan
CXX ?= g++
OUT := _build
CSRC := ../../ptsharp_amd/csrc
ROCM ?= /opt/rocm
HIPINC := -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unknown-pragmas -Wno-attributes
DEPS := query_tables_check.cpp scene_fixture.h $(CSRC)/pt_update_layout.h $(CSRC)/pt_rebuild.h $(CSRC)/pt_refit.h $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_scene_compile.h \
        $(CSRC)/pt_scene.h $(CSRC)/pt_ext.h $(CSRC)/pt_math.h $(CSRC)/pt_bvh.cpp $(CSRC)/pt_bvh.h ../../include/ptsharp_hip.h query.mk
SRC := query_tables_check.cpp $(CSRC)/pt_scene_compile.cpp $(CSRC)/pt_bvh.cpp
FLAGS := -std=c++17 -O2 -ffp-contract=off -fno-fast-math -pthread -Wall $(HIPINC)

query_tables_check: $(OUT)/query_tables_check
asan: $(OUT)/query_tables_check_asan

$(OUT)/query_tables_check: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -o $@ $(SRC)

$(OUT)/query_tables_check_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(FLAGS) -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $(SRC)

.PHONY: query_tables_check asan
