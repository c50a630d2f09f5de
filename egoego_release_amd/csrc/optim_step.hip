// optim_step.hip — host side of the fused parameter update (egoego_optim_*): the layout of the state block and the launch
// sequences over optim_step.h's kernels.  A call only enqueues work on the caller's stream: no allocation, no copy through the
// host and no synchronisation.  The context holds host data only (the element counts and the chunk count).
#include "host_util.h"
#include "optim_step.h"

struct egoego_optim_ctx {
    int device;
    DevMem mem;  // (empty: destroy_ctx's shape)
    std::vector<int64_t> counts, first_chunk;
    int64_t n_chunks;
    bool has_adam = false, has_ema = false;  // what the tables of the last egoego_optim_set_tensors hold
};

namespace {

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout {
    size_t table, chunks, total;
};

Layout layout(const egoego_optim_ctx* c) {
    Layout l;
    l.table = op::HEADER_BYTES;
    l.chunks = l.table + up256(c->counts.size() * sizeof(op::Tensor));
    l.total = l.chunks + up256((size_t)c->n_chunks * sizeof(op::Chunk));
    return l;
}

int check_state(const egoego_optim_ctx* c, const void* d_state, size_t state_bytes) {
    if (!c) return fail(EGOEGO_E_INVALID, "optimizer context is NULL");
    const size_t need = layout(c).total;
    if (!d_state || ((uintptr_t)d_state & 255) || state_bytes < need)
        return fail(EGOEGO_E_WORKSPACE, "state block: %zu bytes at %p, need %zu (256-byte aligned)", state_bytes, d_state, need);
    return 0;
}

}  // namespace

static_assert(sizeof(egoego_optim_state) <= op::HEADER_BYTES, "the state header outgrew its slot");
static_assert(op::CHUNK == EGOEGO_OPTIM_CHUNK && op::CHUNK % 4 == 0, "CHUNK");

extern "C" {

const char* egoego_optim_last_error(void) { return last_err.c_str(); }

int egoego_optim_ctx_create(int device, int n_tensors, const int64_t* counts, egoego_optim_ctx** out) {
    if (!counts || !out) return fail(EGOEGO_E_INVALID, "counts / out is NULL");
    if (n_tensors < 1 || n_tensors > 65536) return fail(EGOEGO_E_INVALID, "n_tensors = %d: 1 .. 65536", n_tensors);
    if (int rc = check_device(device)) return rc;
    int64_t chunks = 0;
    std::vector<int64_t> first(n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
        if (counts[i] < 1) return fail(EGOEGO_E_INVALID, "tensor %d has %lld elements", i, (long long)counts[i]);
        first[i] = chunks;
        chunks += (counts[i] + op::CHUNK - 1) / op::CHUNK;
    }
    if (chunks > ((int64_t)1 << 30)) return fail(EGOEGO_E_INVALID, "%lld chunks: more than 2^30", (long long)chunks);
    egoego_optim_ctx* c = new egoego_optim_ctx();
    c->device = device;
    c->counts.assign(counts, counts + n_tensors);
    c->first_chunk = first;
    c->n_chunks = chunks;
    *out = c;
    return 0;
}

void egoego_optim_ctx_destroy(egoego_optim_ctx* ctx) { destroy_ctx(ctx); }

size_t egoego_optim_workspace_bytes(const egoego_optim_ctx* ctx) {
    if (!ctx) {
        (void)fail(EGOEGO_E_INVALID, "optimizer context is NULL");
        return 0;
    }
    return up256((size_t)ctx->n_chunks * sizeof(double));
}

size_t egoego_optim_state_bytes(const egoego_optim_ctx* ctx) {
    if (!ctx) {
        (void)fail(EGOEGO_E_INVALID, "optimizer context is NULL");
        return 0;
    }
    return layout(ctx).total;
}

int egoego_optim_set_tensors(egoego_optim_ctx* ctx, float* const* p, float* const* g, float* const* m, float* const* v, float* const* ema,
                             void* d_state, size_t state_bytes, void* stream) {
    if (int rc = check_state(ctx, d_state, state_bytes)) return rc;
    if (!p) return fail(EGOEGO_E_INVALID, "the parameter pointers are NULL");
    const bool adam = g || m || v;
    if (adam && !(g && m && v)) return fail(EGOEGO_E_INVALID, "gradients, exp_avg and exp_avg_sq come together or not at all");
    if (!adam && !ema) return fail(EGOEGO_E_INVALID, "neither moments nor EMA tensors: nothing to update");
    const int n = (int)ctx->counts.size();
    for (int i = 0; i < n; ++i) {
        const float* ps[] = {p[i], adam ? g[i] : p[i], adam ? m[i] : p[i], adam ? v[i] : p[i], ema ? ema[i] : p[i]};
        for (const float* q : ps)
            if (!q || ((uintptr_t)q & 3)) return fail(EGOEGO_E_INVALID, "tensor %d: a pointer is NULL or not 4-byte aligned", i);
    }
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    const Layout l = layout(ctx);
    op::Tensor* table = (op::Tensor*)((char*)d_state + l.table);
    op::Chunk* chunks = (op::Chunk*)((char*)d_state + l.chunks);
    for (int first = 0; first < n; first += op::TABLE_BATCH) {
        op::TableArgs a;
        memset(&a, 0, sizeof a);
        a.first = first;
        a.n = n - first < op::TABLE_BATCH ? n - first : op::TABLE_BATCH;
        for (int k = 0; k < a.n; ++k) {
            const int i = first + k;
            a.t[k].p = p[i];
            a.t[k].g = adam ? g[i] : nullptr;
            a.t[k].m = adam ? m[i] : nullptr;
            a.t[k].v = adam ? v[i] : nullptr;
            a.t[k].ema = ema ? ema[i] : nullptr;
            a.t[k].count = ctx->counts[i];
            a.t[k].first_chunk = ctx->first_chunk[i];
        }
        hipLaunchKernelGGL(op::table_kernel, dim3(1), dim3(64), 0, s, a, table);
    }
    hipLaunchKernelGGL(op::chunks_kernel, dim3((unsigned)((ctx->n_chunks + 255) / 256)), dim3(256), 0, s, (const op::Tensor*)table, n, chunks,
                       (int)ctx->n_chunks);
    HIP_TRY(hipGetLastError());
    ctx->has_adam = adam;
    ctx->has_ema = ema != nullptr;
    return 0;
}

int egoego_optimw_step(egoego_optim_ctx* ctx, const egoego_optim_hyper_w* hyper, const egoego_optim_ema* ema, const float* const* losses,
                        int n_losses, const float* d_inv_scale, const float* d_found_inf, int skip_on, int zero_grads, int do_adam, int do_ema,
                        void* d_state, size_t state_bytes, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_state(ctx, d_state, state_bytes)) return rc;
    if (!do_adam && !do_ema) return fail(EGOEGO_E_INVALID, "neither do_adam nor do_ema: nothing to do");
    if (do_adam && !ctx->has_adam) return fail(EGOEGO_E_INVALID, "do_adam: egoego_optim_set_tensors was not given gradients and moments");
    if (do_ema && !ctx->has_ema) return fail(EGOEGO_E_INVALID, "do_ema: egoego_optim_set_tensors was not given EMA tensors");
    if (zero_grads && !do_adam) return fail(EGOEGO_E_INVALID, "zero_grads needs do_adam");
    if (skip_on != EGOEGO_OPTIM_SKIP_NAN && skip_on != EGOEGO_OPTIM_SKIP_NONFINITE) return fail(EGOEGO_E_INVALID, "unknown skip rule %d", skip_on);
    if (n_losses < 0 || n_losses > op::MAX_LOSSES || (n_losses > 0 && !losses))
        return fail(EGOEGO_E_INVALID, "n_losses = %d: 0 .. %d device scalars", n_losses, op::MAX_LOSSES);
    for (int i = 0; i < n_losses; ++i)
        if (!losses[i]) return fail(EGOEGO_E_INVALID, "loss pointer %d is NULL", i);
    if (do_adam) {
        if (!hyper) return fail(EGOEGO_E_INVALID, "do_adam: hyper is NULL");
        if (!(hyper->lr >= 0.0) || !(hyper->eps >= 0.0) || !(hyper->beta1 >= 0.0 && hyper->beta1 < 1.0) ||
            !(hyper->beta2 >= 0.0 && hyper->beta2 < 1.0) || !(hyper->weight_decay >= 0.0))
            return fail(EGOEGO_E_INVALID, "lr %g, betas (%g, %g), eps %g, weight_decay %g: out of range", hyper->lr, hyper->beta1, hyper->beta2,
                        hyper->eps, hyper->weight_decay);
        if (hyper->decoupled != 0 && hyper->decoupled != 1) return fail(EGOEGO_E_INVALID, "decoupled = %d: 0 (L2) or 1 (AdamW)", hyper->decoupled);
        if (hyper->max_norm != hyper->max_norm) return fail(EGOEGO_E_INVALID, "max_norm is NaN (<= 0 turns clipping off)");
        if (!(hyper->clip_eps >= 0.0)) return fail(EGOEGO_E_INVALID, "clip_eps %g: negative or NaN", hyper->clip_eps);
        if (int rc = check_workspace(d_workspace, workspace_bytes, egoego_optim_workspace_bytes(ctx))) return rc;
    }
    if (do_ema) {
        if (!ema || !ema->d_step || !ema->d_initted) return fail(EGOEGO_E_INVALID, "do_ema: the schedule or its counters are NULL");
        if (ema->update_every < 1 || ema->update_after_step < 0 || !(ema->inv_gamma > 0.0) || !(ema->beta >= 0.0 && ema->beta <= 1.0))
            return fail(EGOEGO_E_INVALID, "EMA schedule: update_every %lld, update_after_step %lld, inv_gamma %g, beta %g", (long long)ema->update_every,
                        (long long)ema->update_after_step, ema->inv_gamma, ema->beta);
    }
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    const Layout l = layout(ctx);
    const op::Tensor* table = (const op::Tensor*)((char*)d_state + l.table);
    const op::Chunk* chunks = (const op::Chunk*)((char*)d_state + l.chunks);
    egoego_optim_state* st = (egoego_optim_state*)d_state;
    const int nch = (int)ctx->n_chunks;

    if (do_adam) hipLaunchKernelGGL(op::norm_kernel, dim3(nch), dim3(op::THREADS), 0, s, table, chunks, d_inv_scale, (double*)d_workspace);
    {
        op::Decide a;
        memset(&a, 0, sizeof a);
        a.partial = (const double*)d_workspace;
        a.n_chunks = nch;
        for (int i = 0; i < n_losses; ++i) a.losses[i] = losses[i];
        a.n_losses = n_losses;
        a.found_inf = d_found_inf;
        a.skip_nonfinite = skip_on == EGOEGO_OPTIM_SKIP_NONFINITE;
        a.do_adam = do_adam != 0;
        a.do_ema = do_ema != 0;
        if (do_adam) { a.lr = hyper->lr; a.beta1 = hyper->beta1; a.beta2 = hyper->beta2; a.max_norm = hyper->max_norm; a.clip_eps = hyper->clip_eps; }
        if (do_ema) a.ema = *ema;
        a.st = st;
        hipLaunchKernelGGL(op::decide_kernel, dim3(1), dim3(op::THREADS), 0, s, a);
    }
    {
        op::Apply a;
        memset(&a, 0, sizeof a);
        a.table = table;
        a.chunks = chunks;
        a.n_chunks = nch;
        a.st = st;
        a.inv_scale = d_inv_scale;
        if (do_adam) {
            a.w1 = (float)(1.0 - hyper->beta1);
            a.beta2 = (float)hyper->beta2;
            a.w2 = (float)(1.0 - hyper->beta2);
            a.eps = (float)hyper->eps;
            a.wd = (float)hyper->weight_decay;
            a.wmul = (float)(1.0 - hyper->lr * hyper->weight_decay);  // torch.optim.AdamW's param.mul_(1 - lr * weight_decay)
            a.decoupled = hyper->decoupled;
            a.clip = hyper->max_norm > 0.0;
        }
        a.zero_grads = zero_grads != 0;
        const dim3 grid(nch < op::MAX_BLOCKS ? nch : op::MAX_BLOCKS), block(op::THREADS);
        if (do_adam && do_ema) hipLaunchKernelGGL((op::apply_kernel<true, true>), grid, block, 0, s, a);
        else if (do_adam) hipLaunchKernelGGL((op::apply_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((op::apply_kernel<false, true>), grid, block, 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_optim_step(egoego_optim_ctx* ctx, const egoego_optim_hyper* hyper, const egoego_optim_ema* ema, const float* const* losses,
                      int n_losses, const float* d_inv_scale, const float* d_found_inf, int skip_on, int zero_grads, int do_adam, int do_ema,
                      void* d_state, size_t state_bytes, void* d_workspace, size_t workspace_bytes, void* stream) {
    egoego_optim_hyper_w w;
    memset(&w, 0, sizeof w);  // decoupled = 0, max_norm = 0: the L2 form, no clipping
    if (hyper) { w.lr = hyper->lr; w.beta1 = hyper->beta1; w.beta2 = hyper->beta2; w.eps = hyper->eps; w.weight_decay = hyper->weight_decay; }
    return egoego_optimw_step(ctx, hyper ? &w : nullptr, ema, losses, n_losses, d_inv_scale, d_found_inf, skip_on, zero_grads, do_adam, do_ema,
                               d_state, state_bytes, d_workspace, workspace_bytes, stream);
}

int egoego_optim_read_state(egoego_optim_ctx* ctx, const void* d_state, size_t state_bytes, egoego_optim_state* d_out, void* stream) {
    if (int rc = check_state(ctx, d_state, state_bytes)) return rc;
    if (!d_out) return fail(EGOEGO_E_INVALID, "d_out is NULL");
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    HIP_TRY(hipMemcpyAsync(d_out, d_state, sizeof(egoego_optim_state), hipMemcpyDeviceToDevice, as_stream(stream)));
    return 0;
}

}  // extern "C"
