# Builds the engine library without Python: sage_slam_amd/libsage_ba.so (gfx950 only), the same objects, flags and
# link line as `python -m sage_slam_amd.build` (what __graft_entry__.build() runs).  For a C++ maintainer who wires the
# library into system/sources/cuda/CMakeLists.txt as INTEGRATION.md s1 shows:
#   make -j8            the engine library
#   make oracle         the CPU oracle (test infrastructure; oracle/Makefile)
#   make clean
HIPCC   ?= /opt/rocm/bin/hipcc
HOSTCXX ?= /opt/rocm/lib/llvm/bin/clang++
CSRC    := sage_slam_amd/csrc
OBJ     ?= $(CSRC)/_obj
LIB     ?= sage_slam_amd/libsage_ba.so

HIP_SRC  := photo_kernels.hip geo_kernels.hip track_kernels.hip producers.hip keypoint_kernels.hip graph_kernels.hip solve_kernels.hip \
            operators.hip tracker.hip overlap.hip depth_scale.hip bow.hip registration.hip match_batch.hip voc_build.hip window.hip window_eval.hip window_reduce.hip window_solve.hip window_lm.hip window_profile.hip \
            window_build.hip window_terms.hip window_dist.hip window_factors.hip psd_project.hip window_dogleg.hip window_relin.hip keyframe_prepare.hip window_prior.hip window_covariance.hip depth_sigma.hip tsdf.hip window_tsdf.hip
HOST_SRC := host_math.cpp factor_blocks.cpp block_solver.cpp host_threads.cpp shard_solve.cpp convex_hull.cpp bow_database.cpp registration_host.cpp voc_build_host.cpp depth_scale_host.cpp loop_accept_host.cpp psd_project_host.cpp dogleg_host.cpp relin_host.cpp keyframe_prepare_host.cpp marginal_host.cpp covariance_host.cpp tsdf_host.cpp
HEADERS  := $(addprefix $(CSRC)/,sage_device.h sage_internal.h damped_system.h host_math.h factor_blocks.h block_solver.h host_threads.h device_buffers.h runtime_internal.h window_state.h finalize_bodies.h keypoint_batch.h graph_terms.h graph_batch.h term_results.h window_plan.h registration_plan.h registration_math.h depth_scale_plan.h loop_accept.h voc_build.h psd_project.h dogleg.h relin_plan.h keyframe_prepare.h marginal.h covariance.h tsdf.h) include/sage_ba.h
INC      := -Iinclude -I$(CSRC)
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $(INC)
# pure host translation units: ROCm's clang++ without offload (function multiversioning for AVX2 / AVX-512 inside)
HOSTFLAGS := -O3 -std=c++17 -fPIC -Wall $(INC)

# make CHECK=1 OBJ=/tmp/chk_obj LIB=/tmp/libsage_ba_chk.so : libstdc++'s bounds-checked containers in all host code (the `-m gpu`
# suite runs green on such a build: DESIGN s1 "Sanitizer passes"); point the harness at it with SAGE_BA_LIB=<LIB>
ifdef CHECK
HIPFLAGS  += -D_GLIBCXX_ASSERTIONS
HOSTFLAGS += -D_GLIBCXX_ASSERTIONS
endif

OBJS := $(addprefix $(OBJ)/,$(HIP_SRC:.hip=.o) $(HOST_SRC:.cpp=.o))

.PHONY: lib oracle clean
lib: $(LIB)

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(OBJS) -lpthread

$(OBJ)/%.o: $(CSRC)/%.hip $(HEADERS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OBJ)/%.o: $(CSRC)/%.cpp $(HEADERS) | $(OBJ)
	$(HOSTCXX) $(HOSTFLAGS) -c $< -o $@

$(OBJ):
	mkdir -p $(OBJ)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(OBJ) $(LIB)
