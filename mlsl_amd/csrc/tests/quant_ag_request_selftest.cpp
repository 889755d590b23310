// What a compressed all-gather request refuses at Setup(), on the C++ path
// that the C and Python interfaces cannot reach: an all_gatherv, and any
// element type but f32/bf16, each with an error that names the reason; and
// the request that is accepted reports itself compressed. World 1 over the
// library as built (no sanitizer): RANK=0 WORLD_SIZE=1 MLSL_TRANSPORT=tcp.
// Run by tests/test_quant_ag_cpu.py. Exit 0 = PASS.
#include <cstdio>
#include <string>
#include <vector>

#include "../comm/request.hpp"
#include "../include/mlsl/mlsl.hpp"

using namespace mlsl;

static int g_fail = 0;

static void ExpectThrow(CommRequest& r, const char* needle, const char* what) {
    try {
        r.Setup();
    } catch (const std::exception& e) {
        if (std::string(e.what()).find(needle) == std::string::npos) {
            std::printf("FAIL %s: error does not name the reason: %s\n", what, e.what());
            ++g_fail;
        }
        return;
    }
    std::printf("FAIL %s: Setup() accepted it\n", what);
    ++g_fail;
}

int main(int argc, char** argv) {
    Environment& env = Environment::GetEnv();
    env.Init(&argc, &argv);
    Distribution* dist = env.CreateDistribution(env.GetProcessCount(), 1);
    ProcessGroup* g = dist->Group(GroupKind::DATA);
    const QuantParams qp = env.GetQuantizationParams();
    {
        CommRequest r(g, DataType::F32, CompType::GENERIC);
        r.AddAllGatherv(64, std::vector<size_t>(env.GetProcessCount(), 64));
        r.SetCompression(Compression::QUANT_INT8, qp);
        ExpectThrow(r, "all_gatherv", "quantized all_gatherv");
    }
    {
        CommRequest r(g, DataType::F64, CompType::GENERIC);
        r.AddAllGather(64);
        r.SetCompression(Compression::QUANT_INT8, qp);
        ExpectThrow(r, "f32/bf16", "quantized all_gather of f64");
    }
    for (bool acc : {false, true}) {
        CommRequest r(g, DataType::BF16, CompType::GENERIC);
        r.AddAllGather(64);
        r.SetCompression(Compression::QUANT_INT8, qp);
        r.SetQuantAccumulate(acc);
        r.Setup();
        if (!r.Compressed() || r.Chunks().size() != 1 ||
            r.Chunks()[0].qplan.finish != QuantFinish::SCATTER ||
            r.Chunks()[0].qplan.accumulate != acc || r.Chunks()[0].qplan.residual) {
            std::printf("FAIL accepted request: not the compressed all-gather plan\n");
            ++g_fail;
        }
        bool threw = false;
        try {
            r.SetQuantAccumulate(!acc);
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) {
            std::printf("FAIL SetQuantAccumulate after Setup was accepted\n");
            ++g_fail;
        }
    }
    {
        // an exact all-gather is what it was
        CommRequest r(g, DataType::F64, CompType::GENERIC);
        r.AddAllGather(64);
        r.Setup();
        if (r.Compressed()) {
            std::printf("FAIL exact all-gather reports itself compressed\n");
            ++g_fail;
        }
    }
    env.DeleteDistribution(dist);
    env.Finalize();
    if (g_fail) {
        std::printf("%d FAILURES\n", g_fail);
        return 1;
    }
    std::printf("quant_ag_request_selftest: PASS\n");
    return 0;
}
