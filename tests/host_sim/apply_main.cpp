// apply_kernel of csrc/optim_step.h on the host, under AddressSanitizer and UBSan's alignment check: every view is an allocation of
// exactly its own bytes placed so that it has the 16-byte phase asked for, so a 16-byte access off its boundary or over either end
// of a view stops the program.  Phases 0..3 for all five tensors alike, and each single tensor one element off the other four.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "optim_step.h"

namespace {

struct View {
    float* base;
    float* data;
};

View view(int n, int phase) {  // the allocation ends where the view ends; it begins `phase` elements before it
    void* raw = nullptr;
    if (posix_memalign(&raw, 16, sizeof(float) * (size_t)(n + phase)) != 0) abort();
    View v{(float*)raw, (float*)raw + phase};
    for (int i = 0; i < n + phase; ++i) v.base[i] = 0.f;
    return v;
}

int run_case(const std::vector<int>& counts, const int (*phases)[5], int grid) {
    const int n = (int)counts.size();
    std::vector<op::Tensor> table(n);
    std::vector<op::Chunk> chunks;
    std::vector<View> all;
    for (int t = 0; t < n; ++t) {
        View v[5];
        for (int k = 0; k < 5; ++k) {
            v[k] = view(counts[t], phases[t][k]);
            all.push_back(v[k]);
        }
        for (int i = 0; i < counts[t]; ++i) {
            v[0].data[i] = 0.05f + 0.001f * (float)(i % 7);
            v[1].data[i] = 0.5f - 0.01f * (float)(i % 13);
            v[2].data[i] = 0.01f;
            v[3].data[i] = 0.001f;
            v[4].data[i] = 0.04f;
        }
        table[t] = op::Tensor{v[0].data, v[1].data, v[2].data, v[3].data, v[4].data, counts[t], (int64_t)chunks.size()};
        for (int off = 0; off < counts[t]; off += op::CHUNK)
            chunks.push_back(op::Chunk{t, counts[t] - off < op::CHUNK ? counts[t] - off : op::CHUNK, off});
    }
    egoego_optim_state st;
    memset(&st, 0, sizeof st);
    st.step_size = 1e-3f;
    st.bc2_sqrt = 0.5f;
    st.one_minus_decay = 0.25f;
    st.ema_action = EGOEGO_OPTIM_EMA_LERP;
    op::Apply a;
    memset(&a, 0, sizeof a);
    a.table = table.data();
    a.chunks = chunks.data();
    a.n_chunks = (int)chunks.size();
    a.st = &st;
    a.w1 = 0.1f; a.beta2 = 0.999f; a.w2 = 0.001f; a.eps = 1e-8f; a.wd = 0.01f;
    a.zero_grads = 1;
    gridDim.x = (unsigned)grid;
    blockDim.x = op::THREADS;
    for (unsigned b = 0; b < gridDim.x; ++b)
        for (unsigned t = 0; t < (unsigned)op::THREADS; ++t) {
            blockIdx.x = b;
            threadIdx.x = t;
            op::apply_kernel<true, true>(a);
        }
    int bad = 0;
    for (int t = 0; t < n; ++t)
        for (int i = 0; i < counts[t]; ++i) {
            const float p0 = 0.05f + 0.001f * (float)(i % 7);
            // every element exactly once: the gradient cleared, the moments and the parameter moved, the EMA drawn towards p
            if (table[t].g[i] != 0.f || table[t].m[i] == 0.01f || table[t].v[i] == 0.001f || !(table[t].p[i] < p0) || !(table[t].ema[i] > 0.04f) ||
                !(table[t].ema[i] < table[t].p[i]))
                ++bad;
            const float once = 0.04f - (0.04f - table[t].p[i]) * 0.25f;
            if (std::fabs(table[t].ema[i] - once) > 1e-6f) ++bad;  // (a second visit would draw it twice as far)
        }
    for (const View& v : all) free(v.base);
    return bad;
}

}  // namespace

int main() {
    const std::vector<int> counts = {1, 2, 3, 6, op::CHUNK - 1, op::CHUNK + 2, 2 * op::CHUNK + 5};
    int bad = 0, cases = 0;
    for (int ph = 0; ph < 4; ++ph) {  // one phase for all five
        std::vector<int[5]> phases(counts.size());
        for (auto& p : phases)
            for (int k = 0; k < 5; ++k) p[k] = ph;
        bad += run_case(counts, phases.data(), 3);
        ++cases;
    }
    for (int odd = 0; odd < 5; ++odd)  // one tensor off the others' phase: scalars throughout
        for (int ph = 0; ph < 4; ++ph) {
            std::vector<int[5]> phases(counts.size());
            for (auto& p : phases)
                for (int k = 0; k < 5; ++k) p[k] = k == odd ? (ph + 1) & 3 : ph;
            bad += run_case(counts, phases.data(), 64);
            ++cases;
        }
    printf("%d cases, %d wrong elements\n", cases, bad);
    return bad ? 1 : 0;
}
