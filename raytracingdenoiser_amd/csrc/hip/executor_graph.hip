// HIP executor, graph mode (include/NRDHip.h nrdHipSetGraphMode): the recorded launches of a dispatch range as a cached hipGraph.
#include "executor.h"

using namespace nrdhip;

// Graph mode: the recorded launches of a range as a linear chain of kernel nodes. One executable graph per topology (sequence of kernels);
// on a topology hit only the nodes whose parameters changed (constants, ping-pong planes, row ranges) are updated before the launch.
uint32_t nrdhip::LaunchAsGraph(NrdHipExecutor* e, std::vector<LaunchRecord>& records) {
    if (records.empty())
        return (uint32_t)nrd::Result::SUCCESS;
    std::vector<const void*> funcs(records.size());
    for (size_t i = 0; i < records.size(); i++)
        funcs[i] = records[i].func;
    NrdHipExecutor::CachedGraph* hit = nullptr;
    for (auto& g : e->graphs)
        if (g.funcs == funcs)
            hit = &g;
    std::vector<void*> argPtrs;
    auto paramsOf = [&](LaunchRecord& r) {
        argPtrs.resize(r.offsets.size());
        for (size_t k = 0; k < r.offsets.size(); k++)
            argPtrs[k] = r.args.data() + r.offsets[k];
        hipKernelNodeParams p = {};
        p.func = (void*)r.func;
        p.gridDim = r.grid;
        p.blockDim = r.block;
        p.sharedMemBytes = 0;
        p.kernelParams = argPtrs.data();
        p.extra = nullptr;
        return p;
    };
    if (!hit) {
        if (e->graphs.size() >= 32) { // evict the least recently used topology (a sharded frame is launched as up to ~10 dispatch ranges, each its own topology)
            size_t lru = 0;
            for (size_t i = 1; i < e->graphs.size(); i++)
                if (e->graphs[i].lastUse < e->graphs[lru].lastUse)
                    lru = i;
            // its last launch may still be in flight on the stream: wait before the executable graph goes away (evictions are rare -- 32 topologies)
            (void)hipStreamSynchronize(e->stream);
            (void)hipGraphExecDestroy(e->graphs[lru].exec);
            (void)hipGraphDestroy(e->graphs[lru].graph);
            e->graphs.erase(e->graphs.begin() + (long)lru);
        }
        NrdHipExecutor::CachedGraph g;
        g.funcs = funcs;
        if (hipGraphCreate(&g.graph, 0) != hipSuccess)
            return e->Fail(nrd::Result::FAILURE, "hipGraphCreate failed");
        g.nodes.resize(records.size());
        for (size_t i = 0; i < records.size(); i++) {
            hipKernelNodeParams p = paramsOf(records[i]);
            hipError_t err = hipGraphAddKernelNode(&g.nodes[i], g.graph, i ? &g.nodes[i - 1] : nullptr, i ? 1 : 0, &p);
            if (err != hipSuccess) {
                (void)hipGraphDestroy(g.graph);
                return e->Fail(nrd::Result::FAILURE, std::string("hipGraphAddKernelNode failed: ") + hipGetErrorString(err));
            }
        }
        hipError_t err = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        if (err != hipSuccess) {
            (void)hipGraphDestroy(g.graph);
            return e->Fail(nrd::Result::FAILURE, std::string("hipGraphInstantiate failed: ") + hipGetErrorString(err));
        }
        g.records = records;
        e->graphs.push_back(std::move(g));
        hit = &e->graphs.back();
        e->graphBuilds++;
    } else {
        for (size_t i = 0; i < records.size(); i++) {
            LaunchRecord& have = hit->records[i];
            LaunchRecord& want = records[i];
            const bool same = have.args == want.args && have.grid.x == want.grid.x && have.grid.y == want.grid.y && have.grid.z == want.grid.z && have.block.x == want.block.x &&
                              have.block.y == want.block.y && have.block.z == want.block.z;
            if (same)
                continue;
            hipKernelNodeParams p = paramsOf(want);
            hipError_t err = hipGraphExecKernelNodeSetParams(hit->exec, hit->nodes[i], &p);
            if (err != hipSuccess)
                return e->Fail(nrd::Result::FAILURE, std::string("hipGraphExecKernelNodeSetParams failed: ") + hipGetErrorString(err));
            have = want;
            e->graphNodeUpdates++;
        }
    }
    hit->lastUse = ++e->graphClock;
    hipError_t err = hipGraphLaunch(hit->exec, e->stream);
    if (err != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, std::string("hipGraphLaunch failed: ") + hipGetErrorString(err));
    e->graphLaunches++;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetGraphMode(NrdHipExecutor* e, uint32_t enable) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    e->graphMode = enable != 0;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetGraphStats(const NrdHipExecutor* e, uint64_t* graphLaunches, uint64_t* graphBuilds, uint64_t* nodeUpdates) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (graphLaunches)
        *graphLaunches = e->graphLaunches;
    if (graphBuilds)
        *graphBuilds = e->graphBuilds;
    if (nodeUpdates)
        *nodeUpdates = e->graphNodeUpdates;
    return (uint32_t)nrd::Result::SUCCESS;
}
