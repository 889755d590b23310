# mlsl_amd build: C++17 core + CDNA4 (gfx950) HIP kernels + RCCL, built with
# hipcc into an in-tree shared library the Python ctypes binding loads.
# No MPI, no CUDA, no external deps beyond ROCm.

HIPCC      ?= hipcc
GPU_ARCH   ?= gfx950
BUILD      := build
LIB        := mlsl_amd/libmlsl_amd.so
SELFTEST   := $(BUILD)/schedule_selftest

CXXFLAGS   := -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter \
              --offload-arch=$(GPU_ARCH) -I/opt/rocm/include -MMD -MP
LDFLAGS    := -shared -fPIC -L/opt/rocm/lib -lrccl -lamdhip64 -pthread

CSRC := \
    mlsl_amd/csrc/core/log.cpp \
    mlsl_amd/csrc/core/config.cpp \
    mlsl_amd/csrc/core/sysinfo.cpp \
    mlsl_amd/csrc/core/signals.cpp \
    mlsl_amd/csrc/comm/schedule.cpp \
    mlsl_amd/csrc/comm/quant.cpp \
    mlsl_amd/csrc/comm/quant_plan.cpp \
    mlsl_amd/csrc/comm/device_pool.cpp \
    mlsl_amd/csrc/comm/bootstrap.cpp \
    mlsl_amd/csrc/comm/mesh.cpp \
    mlsl_amd/csrc/comm/group.cpp \
    mlsl_amd/csrc/comm/request.cpp \
    mlsl_amd/csrc/comm/engine.cpp \
    mlsl_amd/csrc/comm/context.cpp \
    mlsl_amd/csrc/comm/p2p_transport.cpp \
    mlsl_amd/csrc/comm/device_comm.cpp \
    mlsl_amd/csrc/dl/environment.cpp \
    mlsl_amd/csrc/dl/rma.cpp \
    mlsl_amd/csrc/dl/session.cpp \
    mlsl_amd/csrc/bind/c_api.cpp \
    mlsl_amd/csrc/bind/ops_api.cpp

HIPSRC := mlsl_amd/csrc/hip/kernels.hip

OBJS := $(CSRC:%.cpp=$(BUILD)/%.o) $(HIPSRC:%.hip=$(BUILD)/%.o)

.PHONY: all lib selftest apitest benchlat samples quantplugin clean test

all: lib selftest apitest e2e benchlat samples quantplugin

lib: $(LIB)

$(LIB): $(OBJS)
	$(HIPCC) $(OBJS) $(LDFLAGS) -o $@

$(BUILD)/%.o: %.cpp
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(BUILD)/%.o: %.hip
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -x hip -c $< -o $@

selftest: $(SELFTEST)

$(SELFTEST): $(BUILD)/mlsl_amd/csrc/tests/schedule_selftest.o $(BUILD)/mlsl_amd/csrc/comm/schedule.o $(BUILD)/mlsl_amd/csrc/core/log.o
	@mkdir -p $(dir $@)
	$(HIPCC) $^ -L/opt/rocm/lib -lamdhip64 -pthread -o $@

APITEST := $(BUILD)/api_selftest

apitest: $(APITEST)

$(APITEST): $(BUILD)/mlsl_amd/csrc/tests/api_selftest.o $(LIB)
	@mkdir -p $(dir $@)
	$(HIPCC) $< -Lmlsl_amd -lmlsl_amd -Wl,-rpath,'$$ORIGIN/../mlsl_amd' -pthread -o $@

E2E := $(BUILD)/mlsl_e2e

e2e: $(E2E)

$(E2E): $(BUILD)/mlsl_amd/csrc/tests/mlsl_e2e.o $(LIB)
	@mkdir -p $(dir $@)
	$(HIPCC) $< -Lmlsl_amd -lmlsl_amd -Wl,-rpath,'$$ORIGIN/../mlsl_amd' -pthread -o $@

BENCHLAT := $(BUILD)/bench_latency

benchlat: $(BENCHLAT)

$(BENCHLAT): $(BUILD)/mlsl_amd/csrc/tests/bench_latency.o $(LIB)
	@mkdir -p $(dir $@)
	$(HIPCC) $< -Lmlsl_amd -lmlsl_amd -Wl,-rpath,'$$ORIGIN/../mlsl_amd' -pthread -o $@

SAMPLES := $(BUILD)/mlsl_sample $(BUILD)/cmlsl_sample

samples: $(SAMPLES)

quantplugin: $(BUILD)/libquant_plugin.so

$(BUILD)/libquant_plugin.so: samples/quant_plugin.c
	@mkdir -p $(dir $@)
	gcc -O2 -shared -fPIC -o $@ $< -lm

$(BUILD)/mlsl_sample: samples/mlsl_sample.cpp $(LIB)
	@mkdir -p $(dir $@)
	$(HIPCC) -O2 -std=c++17 -Imlsl_amd/csrc/include samples/mlsl_sample.cpp \
	    -Lmlsl_amd -lmlsl_amd -Wl,-rpath,'$$ORIGIN/../mlsl_amd' -o $@

$(BUILD)/cmlsl_sample: samples/cmlsl_sample.c $(LIB)
	@mkdir -p $(dir $@)
	gcc -O2 -Imlsl_amd/csrc/include samples/cmlsl_sample.c \
	    -Lmlsl_amd -lmlsl_amd -Wl,-rpath,'$$ORIGIN/../mlsl_amd' -o $@

# Host-logic sanitizer build: the schedule algebra is pure C++ (no HIP), so
# it compiles with g++ + ASan/UBSan — catches indexing/overflow bugs in the
# collective schedules (the reference had no sanitizer integration).
ASAN := $(BUILD)/schedule_selftest_asan

asan: $(ASAN)
	$(ASAN)

$(ASAN): mlsl_amd/csrc/tests/schedule_selftest.cpp mlsl_amd/csrc/comm/schedule.cpp mlsl_amd/csrc/core/log.cpp
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $^ -pthread -o $@

# Compressed collectives under ASan/UBSan: the one-shot reduce-scatter's
# schedule (matching, slot layout, routing), the plan of every compressed
# schedule, and the host codec walked through the exchange by hand over the
# plan's layout. Pure host C++, like the target above.
ASAN_QRS_DIRECT := $(BUILD)/quant_rs_direct_selftest_asan

asan-quant-rs-direct: $(ASAN_QRS_DIRECT)
	$(ASAN_QRS_DIRECT)

$(ASAN_QRS_DIRECT): mlsl_amd/csrc/tests/quant_rs_direct_selftest.cpp mlsl_amd/csrc/comm/schedule.cpp mlsl_amd/csrc/comm/quant.cpp mlsl_amd/csrc/comm/quant_plan.cpp mlsl_amd/csrc/core/log.cpp
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $^ -pthread -ldl -o $@

# The quantized all-gather under ASan/UBSan: its schedule (matching, slots,
# what each send reads), its plan (one segment in, N out, no residual), and
# the host codec walked through the exchange by hand inside plan-sized
# buffers, assigned and accumulated. Pure host C++, like the target above.
ASAN_QAG := $(BUILD)/quant_ag_selftest_asan

asan-quant-ag: $(ASAN_QAG)
	$(ASAN_QAG)

$(ASAN_QAG): mlsl_amd/csrc/tests/quant_ag_selftest.cpp mlsl_amd/csrc/comm/schedule.cpp mlsl_amd/csrc/comm/quant.cpp mlsl_amd/csrc/comm/quant_plan.cpp mlsl_amd/csrc/core/log.cpp
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $^ -pthread -ldl -o $@

# The two-shot quantized allreduce under ASan/UBSan: its schedule (slots,
# routing, the gather, the one SUMQ step), the plan's SUMQ wire table, and the
# host codec walked through both exchanges by hand inside plan-sized buffers.
# Pure host C++, like the targets above.
ASAN_QAR_TWOSHOT := $(BUILD)/quant_ar_twoshot_selftest_asan

asan-quant-ar-twoshot: $(ASAN_QAR_TWOSHOT)
	$(ASAN_QAR_TWOSHOT)

$(ASAN_QAR_TWOSHOT): mlsl_amd/csrc/tests/quant_ar_twoshot_selftest.cpp mlsl_amd/csrc/comm/schedule.cpp mlsl_amd/csrc/comm/quant.cpp mlsl_amd/csrc/comm/quant_plan.cpp mlsl_amd/csrc/core/log.cpp
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $^ -pthread -ldl -o $@

# The codec over a list of tensors under ASan/UBSan: the gather and scatter
# host twins over every segment layout with each tensor an exact-size heap
# allocation, and the ring and two-shot exchanges walked by hand inside
# plan-sized buffers between them, three starts with the residual carried.
# Pure host C++, like the targets above.
ASAN_QSEG := $(BUILD)/quant_seg_selftest_asan

asan-quant-seg: $(ASAN_QSEG)
	$(ASAN_QSEG)

$(ASAN_QSEG): mlsl_amd/csrc/tests/quant_seg_selftest.cpp mlsl_amd/csrc/comm/schedule.cpp mlsl_amd/csrc/comm/quant.cpp mlsl_amd/csrc/comm/quant_plan.cpp mlsl_amd/csrc/core/log.cpp
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $^ -pthread -ldl -o $@

# The reduce-scatter prologue over a list of tensors under ASan/UBSan: the host
# twin over exact-size heap tensors (padding is read through no pointer), and
# the ring and direct exchanges walked by hand inside plan-sized buffers into an
# exact-size recv, three starts with the residual carried. Pure host C++.
ASAN_QRSSEG := $(BUILD)/quant_rs_seg_selftest_asan

asan-quant-rs-seg: $(ASAN_QRSSEG)
	$(ASAN_QRSSEG)

$(ASAN_QRSSEG): mlsl_amd/csrc/tests/quant_rs_seg_selftest.cpp mlsl_amd/csrc/comm/schedule.cpp mlsl_amd/csrc/comm/quant.cpp mlsl_amd/csrc/comm/quant_plan.cpp mlsl_amd/csrc/core/log.cpp
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $^ -pthread -ldl -o $@

# What a compressed all-gather request refuses at Setup(), through the C++
# classes and the library as built (no sanitizer; world 1 over TCP).
QAG_REQUEST := $(BUILD)/quant_ag_request_selftest

quant-ag-request: $(QAG_REQUEST)

$(QAG_REQUEST): mlsl_amd/csrc/tests/quant_ag_request_selftest.cpp $(LIB)
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 $< -Lmlsl_amd -lmlsl_amd \
	    -Wl,-rpath,'$$ORIGIN/../mlsl_amd' -pthread -o $@

# Full-stack ASan: the API selftest (planner+engine+mesh, TCP world
# matrix) host-compiled with g++ + ASan/UBSan; device kernels stubbed.
ASAN_API := $(BUILD)/api_selftest_asan
ASAN_SRC := $(CSRC) mlsl_amd/csrc/tests/api_selftest.cpp mlsl_amd/csrc/tests/asan_kernel_stubs.cpp

asan-api: $(ASAN_API)

$(ASAN_API): $(ASAN_SRC)
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include 	    -fsanitize=address,undefined -fno-omit-frame-pointer 	    $(ASAN_SRC) -L/opt/rocm/lib -lrccl -lamdhip64 -pthread -o $@

# The IPC-window schedule walker's launch sequence under ASan/UBSan: the real
# schedules and plans through P2pGroup::IssueSchedule on a hand-built group,
# every launcher recording its arguments (asan_kernel_stubs.cpp). Prints one
# digest line per case and rank; tests/golden/p2p_issue_trace.txt pins them.
P2P_TRACE := $(BUILD)/p2p_issue_trace_asan
P2P_TRACE_SRC := $(CSRC) mlsl_amd/csrc/tests/p2p_issue_trace.cpp \
    mlsl_amd/csrc/tests/asan_kernel_stubs.cpp

p2p-trace: $(P2P_TRACE)

$(P2P_TRACE): $(P2P_TRACE_SRC)
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
	    -fsanitize=address,undefined -fno-omit-frame-pointer \
	    $(P2P_TRACE_SRC) -L/opt/rocm/lib -lrccl -lamdhip64 -pthread -o $@

TSAN_API := $(BUILD)/api_selftest_tsan

tsan-api: $(TSAN_API)

$(TSAN_API): $(ASAN_SRC)
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
	    -fsanitize=thread -fno-omit-frame-pointer \
	    $(ASAN_SRC) -L/opt/rocm/lib -lrccl -lamdhip64 -pthread -o $@

# Concurrent-submit race test (multi-producer MPSC ring) under TSan.
TSAN_SUBMIT := $(BUILD)/submit_race_tsan
TSAN_SUBMIT_SRC := $(CSRC) mlsl_amd/csrc/tests/submit_race_selftest.cpp \
    mlsl_amd/csrc/tests/asan_kernel_stubs.cpp

tsan-submit: $(TSAN_SUBMIT)

$(TSAN_SUBMIT): $(TSAN_SUBMIT_SRC)
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
	    -fsanitize=thread -fno-omit-frame-pointer \
	    $(TSAN_SUBMIT_SRC) -L/opt/rocm/lib -lrccl -lamdhip64 -pthread -o $@

test: all samples
	$(SELFTEST)
	python -m pytest tests/ -x -q -m "not gpu"

clean:
	rm -rf $(BUILD) $(LIB)

-include $(OBJS:.o=.d)
-include $(BUILD)/mlsl_amd/csrc/tests/schedule_selftest.d
-include $(BUILD)/mlsl_amd/csrc/tests/api_selftest.d
-include $(BUILD)/mlsl_amd/csrc/tests/bench_latency.d
-include $(BUILD)/mlsl_amd/csrc/tests/mlsl_e2e.d
