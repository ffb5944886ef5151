// pj_blocked_lab.inc -- functions of the development build (-DTETSIM_ABLATION) of pj_blocked.hip; EMPTY in the product build.
// Included inside namespace tetsim { namespace { ... right behind pj_math.inc.  See pj_lab.h.
#ifdef TETSIM_ABLATION
// Development (TETSIM_DEBUG_ITER_HIST; tools/attic/rotation_iterations.py): what a tet's nine |omega|^2 say about exit thresholds.  For each of
// the thresholds {1e-9 (the reference's), 1e-7, 3e-7, 1e-6} the number of iterations this tet (level 0) and its whole wave (level 1:
// the loop is wave-uniform) would execute if the correction iterations 2..9 ended at that threshold -- iteration 1 always uses 1e-9 --
// and the distribution of |omega| per iteration in half decades.  hist: [2][4][10] counts by iterations executed (1..9), then
// [9][22] half-decade bins (bin 0: < 1e-10 incl. "done", bin 21: >= 1).
__device__ __forceinline__ void pjb_log_iterations(unsigned long long* hist, const float* w2log) {
    const float thr2[4] = {1.0e-18f, 1.0e-14f, 9.0e-14f, 1.0e-12f};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int n = 9;
#pragma unroll
        for (int j = 8; j >= 0; j--) {   // the first iteration whose omega fails the test ends the loop (computed, not applied)
            const float lim = j == 0 ? 1.0e-18f : thr2[k];
            if (w2log[j] < lim) n = j + 1;   // (-1 = not executed: done)
        }
        atomicAdd(&hist[(0 * 4 + k) * 10 + n], 1ull);
        int wn = n;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wn = max(wn, __shfl_xor(wn, o));   // (lanes without a tet are not here: the tail wave of a tile under-reports by its idle lanes only)
        if ((threadIdx.x & 63u) == static_cast<uint32_t>(__ffsll(static_cast<long long>(__builtin_amdgcn_ballot_w64(true))) - 1)) atomicAdd(&hist[(1 * 4 + k) * 10 + wn], 1ull);
    }
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const float w = w2log[j] > 0.0f ? sqrtf(w2log[j]) : 0.0f;
        int bin = w > 0.0f ? static_cast<int>(floorf(2.0f * log10f(w))) + 21 : 0;   // 1e-10 -> 1, 1 -> 21
        bin = min(max(bin, 0), 21);
        atomicAdd(&hist[80 + j * 22 + bin], 1ull);
    }
}

// the run-time mode word of the development build's tet kernels (unset => 9 iterations, peeled, all stores)
static uint32_t tet_mode() {
    static int dbg = -1;
    if (dbg < 0) {  // timing ablations (see the kernel comment); unset => 9 iterations, peeled, all stores
        const char* it = getenv("TETSIM_DEBUG_ITERS");
        const char* sk = getenv("TETSIM_DEBUG_SKIP_REST_STORE");
        const char* np = getenv("TETSIM_DEBUG_NO_PEEL");
        const char* sg = getenv("TETSIM_DEBUG_STAGGER");
        const char* sm = getenv("TETSIM_DEBUG_STAGGER_MAP");
        const char* pt = getenv("TETSIM_DEBUG_POLL_TRACE");   // (tetsim_create.hip sizes the trace for the rows of the looks)
        dbg = (it ? (atoi(it) & 15) : 9) | ((sk && sk[0] == '1') ? 16 : 0) | ((np && np[0] == '1') ? 64 : 0) | (sg ? ((atoi(sg) & 255) << 8) : 0) |
              ((sm && sm[0] == '1') ? 0x10000 : 0) | (pt ? 0x20000 : 0);
        fprintf(stderr, "[tetsim] WARNING: ABLATION build of libtetsim_hip (mode 0x%x): timing experiments only, the results are NOT the solver's\n", dbg);
    }
    return static_cast<uint32_t>(dbg);
}
#endif
