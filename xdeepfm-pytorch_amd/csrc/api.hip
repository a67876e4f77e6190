// Error text, tuning options and small host-side entry points of libxdfm_hip.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "xdfm_internal.h"
#include "finish_batch.h"

static thread_local char g_err[512] = "";
static int g_opts[OPT_COUNT] = {
    /* OPT_FWD_NF */ 1,
    /* OPT_BWW_NSPLIT */ 0,
    /* OPT_BWW_SLAB */ 1,
    /* OPT_BWW_MT */ 0,
    /* OPT_DBG */ 0,
    /* OPT_CIN_MATH */ 1,
    /* OPT_X3_FWD_MT */ 0,
    /* OPT_X3_BWX_ROWS */ 0,
    /* OPT_X3_WAVES */ 0,
    /* OPT_BWW_PHASE */ 0,
    /* OPT_ADAM_BX */ 0,
    /* OPT_LAST_FWD */ -1,
    /* OPT_LAST_BWX */ -1,
    /* OPT_LAST_BWW */ -1,
    /* OPT_LAST_SYM */ 0,
    /* OPT_X3_SYM */ 1,
    /* OPT_BWW_XCD */ 1,
    /* OPT_LAST_FWD_INST */ -1,
    /* OPT_LAST_BWX_INST */ -1,
    /* OPT_LAST_BWW_INST */ -1,
    /* OPT_LAST_FWD_F32 */ -1,
    /* OPT_LAST_BWX_F32 */ -1,
    /* OPT_LAST_BWW_F32 */ -1,
    /* OPT_ADAM_ROWS */ 1,
    /* OPT_LAST_ADAM_ROWS */ -1,
    /* OPT_OPT_BX */ 0,
    /* OPT_FINISH_BATCH */ 1,
    /* OPT_COLAUNCH */ 7,
    /* OPT_LAST_COLAUNCH */ -1,
    /* OPT_LAST_RIDERS */ -1,
    /* OPT_LAST_PACK_RIDERS */ -1,
};
static const char* const g_opt_names[OPT_COUNT] = {"fwd_nf", "bww_nsplit", "bww_slab", "bww_mt", "dbg", "cin_math", "x3_fwd_mt", "x3_bwx_rows", "x3_waves", "bww_phase", "adam_bx", "last_fwd_kernel", "last_bwx_kernel", "last_bww_kernel", "last_sym", "x3_sym", "bww_xcd", "last_fwd_inst", "last_bwx_inst", "last_bww_inst", "last_fwd_f32", "last_bwx_f32", "last_bww_f32", "adam_rows", "last_adam_rows", "opt_bx", "finish_batch", "colaunch", "last_colaunch", "last_riders", "last_pack_riders"};

int xdfm_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int xdfm_opt(int idx) { return g_opts[idx]; }

#define XDFM_MAX_DEVICES 16
void xdfm_opt_note(int idx, int value) { g_opts[idx] = value; }

// ---- finish batch (finish_batch.h) -------------------------------------------------------------------------------------
// One launch for the finishes a batch collected.  The job table travels in the kernel arguments (as AdamBatch and X3PackJobs
// do): no host-to-device copy and no memset, so the launch can be captured in a graph.  A workgroup finds its job in the
// prefix table `first` and runs the family's body with the workgroup index it would have had in the family's own launch.
__global__ __launch_bounds__(FINISH_THREADS) void finish_multi_kernel(const FinishTable tab) {
    __shared__ float smf[FINISH_THREADS];
    __shared__ double smd[4];
    int ji = 0;
#pragma unroll
    for (int k = 1; k < FINISH_MAX_JOBS; ++k) ji += (int)blockIdx.x >= tab.first[k] ? 1 : 0;      // first[k >= n] = the grid
    const FinishJob& j = tab.j[ji];
    const int lb = (int)blockIdx.x - tab.first[ji];
    bool scalar_out = false;                       // thread 0 has left the job's single value in out[0]: the tails follow
    switch (j.kind) {                              // uniform over the workgroup
        case FJ_CIN_DBIAS:
            cin_dbias_finish_row(lb * FINISH_THREADS + (int)threadIdx.x, (const float*)j.part, j.i0, j.i1, (float*)j.out, j.i2 != 0);
            break;
        case FJ_DENSE_W:
            if (lb < j.i1) dn_finish_elem((long)lb * FINISH_THREADS + threadIdx.x, (const float*)j.part, j.i0, j.n0, j.n1, (float*)j.out, (float*)j.out2);
            else dn_dalpha_finish_block((const double*)j.part2, j.i2, (float*)j.out3, smd);
            break;
        case FJ_COLSUM:
            colsum_finish_block(lb, (const float*)j.part, j.i0, (float*)j.out, smf);
            break;
        case FJ_HEAD_FWD:
            head_fwd_finish_block((const float*)j.part, smf);
            if (threadIdx.x == 0) ((float*)j.out)[0] = smf[0];
            scalar_out = true;
            break;
        case FJ_HEAD_BWD:
            head_bwd_finish_elem(lb * FINISH_THREADS + (int)threadIdx.x, (const float*)j.part, j.i0, (float*)j.out);
            break;
        case FJ_ADAM_L2:
            adam_l2_finish_block<FINISH_THREADS>((const float*)j.part, j.i0, smf);
            if (threadIdx.x == 0) {
                ((float*)j.out)[0] = smf[0];
                if (j.cell) adam_rows_finish_one(j.cell, (float*)j.out);
            }
            scalar_out = true;
            break;
        case FJ_ADAM_ROWS:
            if (threadIdx.x == 0) adam_rows_finish_one(j.cell, (float*)j.out);
            scalar_out = true;
            break;
        default:                                   // FJ_ADD: the tail alone
            scalar_out = true;
            break;
    }
    if (scalar_out && threadIdx.x == 0 && j.add_out) j.add_out[0] = j.add_a[0] + j.add_b[0];
}

struct FinishBatch {
    std::vector<FinishJob> jobs;
    hipStream_t st = nullptr;
};
static FinishBatch g_finish[XDFM_MAX_DEVICES];
static int g_finish_dev = -1;                      // the device whose batch is open; -1: none

static bool finish_job_writes(const FinishJob& j, const void* p) {
    return p && (j.out == p || j.out2 == p || j.out3 == p || (const void*)j.add_out == p || (const void*)j.cell == p);
}

// launches the collected jobs, FINISH_MAX_JOBS to a launch
static int finish_launch_pending(FinishBatch& fb) {
    const size_t n = fb.jobs.size();
    for (size_t j0 = 0; j0 < n; j0 += FINISH_MAX_JOBS) {
        FinishTable tab;
        memset(&tab, 0, sizeof(tab));
        tab.n = (int)(n - j0 < FINISH_MAX_JOBS ? n - j0 : FINISH_MAX_JOBS);
        // the jobs of few workgroups first: they are the ones that add a long row of partials in one thread, and should not
        // wait behind the wide jobs' workgroups for a slot (jobs of one launch do not depend on each other)
        std::stable_sort(fb.jobs.begin() + j0, fb.jobs.begin() + j0 + tab.n,
                         [](const FinishJob& a, const FinishJob& b) { return a.blocks < b.blocks; });
        int blocks = 0;
        for (int k = 0; k < tab.n; ++k) {
            tab.j[k] = fb.jobs[j0 + k];
            tab.first[k] = blocks;
            blocks += tab.j[k].blocks;
        }
        for (int k = tab.n; k <= FINISH_MAX_JOBS; ++k) tab.first[k] = blocks;
        if (blocks > 0) hipLaunchKernelGGL(finish_multi_kernel, dim3(blocks), dim3(FINISH_THREADS), 0, fb.st, tab);
    }
    fb.jobs.clear();
    return xdfm_check_launch("finish_batch");
}

int xdfm_finish_defer(const FinishJob& job, hipStream_t st, bool* taken) {
    *taken = false;
    if (g_finish_dev < 0) return XDFM_OK;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != g_finish_dev)
        return xdfm_fail(XDFM_ERR_INVALID, "finish batch: opened on device %d, a finish arrives on device %d", g_finish_dev, dev);
    FinishBatch& fb = g_finish[dev];
    if (fb.jobs.empty()) fb.st = st;
    else if (fb.st != st)
        return xdfm_fail(XDFM_ERR_INVALID, "finish batch: a finish arrives on stream %p, the batch collects on stream %p", (void*)st, (void*)fb.st);
    XDFM_REQUIRE(job.blocks > 0 && job.kind >= 0 && job.kind < FJ_KINDS, "finish batch: bad job (kind %d, %d workgroups)", job.kind, job.blocks);
    *taken = true;
    // finishes that feed each other share a launch as tails of the job they follow
    if (job.kind == FJ_ADAM_ROWS && job.out)
        for (size_t k = fb.jobs.size(); k-- > 0;)
            if (fb.jobs[k].kind == FJ_ADAM_L2 && fb.jobs[k].out == job.out && !fb.jobs[k].cell && !fb.jobs[k].add_out) {
                fb.jobs[k].cell = job.cell;
                return XDFM_OK;
            }
    if (job.kind == FJ_ADD)
        for (size_t k = fb.jobs.size(); k-- > 0;) {
            FinishJob& p = fb.jobs[k];
            if ((p.kind == FJ_ADAM_L2 || p.kind == FJ_ADAM_ROWS) && p.out && p.out == (const void*)job.add_b && !p.add_out &&
                !finish_job_writes(p, job.add_a)) {
                p.add_a = job.add_a; p.add_b = job.add_b; p.add_out = job.add_out;
                return XDFM_OK;
            }
        }
    // a job that reads what a collected job still has to write cannot run beside it: the collected ones go first
    const void* reads[4] = {nullptr, nullptr, nullptr, nullptr};
    if (job.kind == FJ_ADAM_ROWS) { reads[0] = job.out; reads[1] = job.cell; }
    if (job.kind == FJ_ADD) { reads[0] = job.add_a; reads[1] = job.add_b; }
    if (job.kind == FJ_CIN_DBIAS && !job.i2) reads[0] = job.out;
    reads[2] = job.out; reads[3] = job.add_out;    // nor write what a collected job writes
    bool clash = false;
    for (const FinishJob& p : fb.jobs)
        for (const void* r : reads) clash = clash || finish_job_writes(p, r);
    if (clash)
        if (int rc = finish_launch_pending(fb)) return rc;
    fb.jobs.push_back(job);
    return XDFM_OK;
}

__global__ void finish_add_kernel(const float* a, const float* b, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = a[0] + b[0];
}

extern "C" {

int xdfm_abi_version(void) { return XDFM_ABI_VERSION; }

const char* xdfm_last_error(void) { return g_err; }

int xdfm_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    return e == hipSuccess ? n : -(int)e;
}

int xdfm_graph_node_census(void* graph, int* n_nodes, int* n_memset, int* n_unexpected) {
    if (!graph || !n_nodes || !n_memset || !n_unexpected) return xdfm_fail(XDFM_ERR_INVALID, "graph_node_census: null pointer");
    size_t n = 0;
    hipError_t e = hipGraphGetNodes((hipGraph_t)graph, nullptr, &n);
    if (e != hipSuccess) return xdfm_fail(XDFM_ERR_LAUNCH, "hipGraphGetNodes: %s", hipGetErrorString(e));
    hipGraphNode_t* nodes = (hipGraphNode_t*)malloc((n ? n : 1) * sizeof(hipGraphNode_t));
    if (!nodes) return xdfm_fail(XDFM_ERR_LAUNCH, "graph_node_census: out of host memory");
    e = hipGraphGetNodes((hipGraph_t)graph, nodes, &n);
    int ms = 0, other = 0;
    for (size_t i = 0; e == hipSuccess && i < n; ++i) {
        hipGraphNodeType t;
        e = hipGraphNodeGetType(nodes[i], &t);
        if (e != hipSuccess) break;
        if (t == hipGraphNodeTypeMemset) ++ms;
        else if (t != hipGraphNodeTypeKernel && t != hipGraphNodeTypeMemcpy && t != hipGraphNodeTypeEmpty &&
                 t != hipGraphNodeTypeWaitEvent && t != hipGraphNodeTypeEventRecord) ++other;
    }
    free(nodes);
    if (e != hipSuccess) return xdfm_fail(XDFM_ERR_LAUNCH, "graph_node_census: %s", hipGetErrorString(e));
    *n_nodes = (int)n; *n_memset = ms; *n_unexpected = other;
    return XDFM_OK;
}

int xdfm_finish_batch_begin(void) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return xdfm_fail(XDFM_ERR_NO_DEVICE, "finish_batch_begin: %s", hipGetErrorString(e));
    if (dev < 0 || dev >= XDFM_MAX_DEVICES) return xdfm_fail(XDFM_ERR_INVALID, "finish_batch_begin: device %d", dev);
    if (g_finish_dev == dev) return xdfm_fail(XDFM_ERR_INVALID, "finish_batch_begin: a batch is open already (xdfm_finish_batch_run closes it)");
    if (g_finish_dev >= 0)
        return xdfm_fail(XDFM_ERR_INVALID, "finish_batch_begin: device %d, but the batch opened on device %d is not closed", dev, g_finish_dev);
    if (!g_opts[OPT_FINISH_BATCH]) return XDFM_OK;         // switched off: no batch, every finish stays its own launch
    g_finish[dev].jobs.clear();
    g_finish[dev].st = nullptr;
    g_finish_dev = dev;
    return XDFM_OK;
}

int xdfm_finish_batch_active(void) {
    int dev = -1;
    return (g_finish_dev >= 0 && hipGetDevice(&dev) == hipSuccess && dev == g_finish_dev) ? 1 : 0;
}

int xdfm_finish_batch_run(void* stream) {
    if (g_finish_dev < 0) return XDFM_OK;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != g_finish_dev)
        return xdfm_fail(XDFM_ERR_INVALID, "finish_batch_run: the batch was opened on device %d, this is device %d", g_finish_dev, dev);
    FinishBatch& fb = g_finish[dev];
    if (!fb.jobs.empty() && fb.st != (hipStream_t)stream)
        return xdfm_fail(XDFM_ERR_INVALID, "finish_batch_run: stream %p, the jobs were recorded on stream %p", stream, (void*)fb.st);
    g_finish_dev = -1;
    return fb.jobs.empty() ? XDFM_OK : finish_launch_pending(fb);
}

int xdfm_finish(int kind, const void* part, const void* part2, void* out, void* out2, void* out3, long n0, long n1, int i0, int i1,
                void* stream) {
    hipStream_t st = (hipStream_t)stream;
    XDFM_REQUIRE(kind >= 0 && kind < FJ_KINDS, "xdfm_finish: kind %d", kind);
    XDFM_REQUIRE(kind == FJ_ADAM_ROWS || (part && out), "xdfm_finish: null pointer");
    int rc = XDFM_OK;
    switch (kind) {
        case FJ_CIN_DBIAS:
            XDFM_REQUIRE(i0 > 0 && i1 > 0, "xdfm_finish: dbias of H = %d rows from %d partials each", i0, i1);
            rc = xdfm_cin_dbias_finish((const float*)part, i0, i1, (float*)out, st);
            break;
        case FJ_DENSE_W:
            XDFM_REQUIRE(n0 > 0 && n1 > 0 && i0 >= 1 && i0 <= DN_MAX_SPLIT && i1 >= 0 && (!out3 || part2),
                         "xdfm_finish: dense dW of (%ld, %ld), %d splits, %d slope partials", n0, n1, i0, i1);
            rc = xdfm_dense_w_finish((const float*)part, i0, n0 * n1, n0, (float*)out, (float*)out2, part2 != nullptr, (const double*)part2, i1,
                                     (float*)out3, st);
            break;
        case FJ_COLSUM:
            XDFM_REQUIRE(i0 > 0, "xdfm_finish: %d columns", i0);
            rc = xdfm_colsum_finish((const float*)part, i0, (float*)out, st);
            break;
        case FJ_HEAD_FWD: rc = xdfm_head_fwd_finish((const float*)part, (float*)out, st); break;
        case FJ_HEAD_BWD:
            XDFM_REQUIRE(i0 > 0, "xdfm_finish: KT = %d", i0);
            rc = xdfm_head_bwd_finish((const float*)part, i0, (float*)out, st);
            break;
        case FJ_ADAM_L2:
            XDFM_REQUIRE(i0 > 0, "xdfm_finish: %d partials", i0);
            rc = xdfm_adam_l2_finish((const float*)part, i0, (float*)out, st);
            break;
        case FJ_ADAM_ROWS:
            XDFM_REQUIRE(out2 && (((size_t)out2) & 7) == 0, "xdfm_finish: the cell must be an 8-byte aligned pointer");
            rc = xdfm_adam_rows_finish((unsigned long long*)out2, (float*)out, st);
            break;
        default: {
            XDFM_REQUIRE(part2, "xdfm_finish: null pointer");
            FinishJob j{};
            j.kind = FJ_ADD; j.blocks = 1;
            j.add_a = (const float*)part; j.add_b = (const float*)part2; j.add_out = (float*)out;
            bool taken = false;
            rc = xdfm_finish_defer(j, st, &taken);
            if (!rc && !taken) hipLaunchKernelGGL(finish_add_kernel, dim3(1), dim3(64), 0, st, j.add_a, j.add_b, j.add_out);
        }
    }
    if (rc) return rc;
    return xdfm_check_launch("xdfm_finish");
}

int xdfm_set_option(const char* key, int value) {
    if (!key) return xdfm_fail(XDFM_ERR_INVALID, "xdfm_set_option: null key");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (strcmp(key, g_opt_names[i]) == 0) {
            g_opts[i] = value;
            return XDFM_OK;
        }
    return xdfm_fail(XDFM_ERR_INVALID, "xdfm_set_option: unknown key '%s'", key);
}

int xdfm_get_option(const char* key) {
    if (!key) return -1;
    for (int i = 0; i < OPT_COUNT; ++i)
        if (strcmp(key, g_opt_names[i]) == 0) return g_opts[i];
    return -1;
}

}  // extern "C"
