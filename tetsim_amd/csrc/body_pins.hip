// body_pins.hip -- many held particles per body of a batch (tetsim_set_body_pins / _device).  What the particle passes read (dev_common.h:
// body_hold_row, the second mode of the body grabs' branch) is made here: per particle in DEVICE particle order the row that holds it
// (-1 = free), and per_body rows of 16 bytes per body, {device particle or -1, target xyz} -- body_grabs.hip's row.  A set call is three
// small kernels on the handle's stream: free the slots of the bodies it takes, scatter the valid rows' indices with an integer minimum (the
// lowest row of a particle wins, whatever order the lanes run in: two calls give the same bits), write the normalised rows.  The host
// steps are body_rows.h's (set_rows_device, launch_row_chunks), shared with the other per-body tables; the normalisation's statement on the
// host is tetsim_prep_pin_slots (tetsim_host.cpp), which the host variant calls and tests/test_body_pins_cpu.py restates.  See body.h.
#include "body_rows.h"

using namespace tetsim;

namespace tetsim {

const char* const kBodyPinsOn = "body pins are on (tetsim_set_body_pins): one kind of hold at a time -- switch them off first";

namespace {

constexpr int32_t kFree = -1;
__host__ __device__ inline int4 no_row() { return make_int4(-1, 0, 0, 0); }

// One lane per particle (device order): the slots of the bodies the call takes go back to "free".  body: the particle -> body array.
__global__ __launch_bounds__(256) void pin_clear_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ body, int32_t* __restrict__ slot, uint32_t nv) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    if (mask && mask[body[v]] == 0) return;
    slot[v] = kFree;
}
// every row to "none"
__global__ __launch_bounds__(256) void pin_rows_none_kernel(int4* __restrict__ rows, uint32_t total) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < total) rows[r] = no_row();
}

// The caller's row r -> the table's, or "none": an index outside the body, a non-finite target.  first[b]: the body's first particle in the
// caller's numbering; map: caller's particle -> device particle (null = identity).  Both kernels below read a row through this.
__device__ __forceinline__ int4 pin_row(const int32_t* __restrict__ particles, const char* __restrict__ targets, uint64_t stride, const uint32_t* __restrict__ first,
                                        const uint32_t* __restrict__ map, uint32_t b, uint32_t r) {
    const int32_t p = particles[r];
    const float* const t = reinterpret_cast<const float*>(targets + static_cast<uint64_t>(r) * stride);
    const float x = t[0], y = t[1], z = t[2];
    const uint32_t f0 = first[b], n = first[b + 1u] - f0;
    if (!(p >= 0 && static_cast<uint32_t>(p) < n && finite_f32(x) && finite_f32(y) && finite_f32(z))) return no_row();
    const uint32_t a = f0 + static_cast<uint32_t>(p);   // (< first[b + 1] <= particles of the handle: the slot it indexes exists)
    return make_int4(static_cast<int32_t>(map ? map[a] : a), __float_as_int(x), __float_as_int(y), __float_as_int(z));
}
// One lane per row: a valid row bids for its particle's slot with its own index.  A free slot is -1, the largest unsigned value, and a
// row index is below 2^31: the unsigned minimum is the lowest bidding row, and non-negative as the int32 the passes read.
__global__ __launch_bounds__(256) void pin_scatter_kernel(const int32_t* __restrict__ particles, const char* __restrict__ targets, uint64_t stride,
                                                          const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first, const uint32_t* __restrict__ map,
                                                          int32_t* __restrict__ slot, uint32_t per_body, uint32_t total) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= total) return;
    const uint32_t b = r / per_body;
    if (mask && mask[b] == 0) return;
    const int4 row = pin_row(particles, targets, stride, first, map, b, r);
    if (row.x >= 0) atomicMin(reinterpret_cast<uint32_t*>(slot) + row.x, r);
}
// One lane per row, behind the scatter: the row as the table holds it -- the winner of its particle's slot, or "none".  A body the mask
// leaves out keeps its rows.
__global__ __launch_bounds__(256) void pin_rows_kernel(const int32_t* __restrict__ particles, const char* __restrict__ targets, uint64_t stride,
                                                       const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first, const uint32_t* __restrict__ map,
                                                       const int32_t* __restrict__ slot, int4* __restrict__ rows, uint32_t per_body, uint32_t total) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= total) return;
    const uint32_t b = r / per_body;
    if (mask && mask[b] == 0) return;
    int4 row = pin_row(particles, targets, stride, first, map, b, r);
    if (row.x >= 0 && slot[row.x] != static_cast<int32_t>(r)) row = no_row();
    rows[r] = row;
}
// The host variant's rows travel as kernel arguments, a chunk per launch, normalised and translated on the host: a row that holds a
// particle is the only one to name it, so the slots need no minimum here.
constexpr uint32_t kRowsPerLaunch = 128;
using Chunk = RowChunk<int4, 1u, kRowsPerLaunch>;
__global__ __launch_bounds__(kRowsPerLaunch) void pin_rows_value_kernel(Chunk c, int4* __restrict__ rows, int32_t* __restrict__ slot, uint32_t first, uint32_t count) {
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    const int4 row = c.row[i][0];
    rows[first + i] = row;
    if (row.x >= 0) slot[row.x] = static_cast<int32_t>(first + i);
}

uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

// every slot free (mask null) or those of the bodies a call takes, on h->stream
void launch_clear(tetsim_body* h, const uint8_t* mask) {
    const uint32_t nv = h->info.num_particles;
    if (nv) hipLaunchKernelGGL(pin_clear_kernel, dim3(blocks_of(nv)), dim3(256), 0, h->stream, mask, h->d_grab_body, h->d_pin_slot, nv);
}
// the whole table empty, on h->stream
int launch_empty_table(tetsim_body* h) {
    const uint32_t total = num_bodies(h) * h->pin_per_body;
    launch_clear(h, nullptr);
    if (total) hipLaunchKernelGGL(pin_rows_none_kernel, dim3(blocks_of(total)), dim3(256), 0, h->stream, h->d_pin_rows, total);
    return launched(h);
}

// The table for `per_body` rows per body.  The first call allocates the slots and the rows (it may block); a call with another per_body
// makes the rows anew -- it waits for the kernels that may still read the old ones before they are released, and the table starts empty.
int ensure_pin_table(tetsim_body* h, uint32_t per_body) {
    if (int rc = ensure_particle_bodies(h)) return rc;
    bool empty = false;
    if (!h->d_pin_slot) {
        if (int rc = dev_alloc(h, &h->d_pin_slot, h->info.num_particles)) return rc;
        empty = true;
    }
    if (!h->d_pin_rows || per_body != h->pin_per_body) {
        const size_t total = static_cast<size_t>(num_bodies(h)) * per_body;
        if (h->d_pin_rows && total > h->pin_rows_cap) HIPCHK(h, hipStreamSynchronize(h->stream));
        if (int rc = dev_grow(h, &h->d_pin_rows, &h->pin_rows_cap, total)) { h->body_pins_on = false; h->pin_per_body = 0; return rc; }
        h->pin_per_body = per_body;
        empty = true;
    }
    return empty ? launch_empty_table(h) : 0;
}

int check_per_body(tetsim_body* h, uint32_t per_body) {
    if (per_body == 0u) return fail(h, TETSIM_EINVAL, "per_body must be at least 1");
    if (static_cast<uint64_t>(per_body) * num_bodies(h) >= 0x80000000ull) return fail(h, TETSIM_EINVAL, "per_body * num_bodies must be below 2^31");
    return 0;
}
// what either set call refuses whatever its rows are
int check_pin_state(tetsim_body* h) {
    if (h->partitioned || !h->group.empty()) return fail(h, TETSIM_ESTATE, "body pins on a partitioned body are not supported");
    if (h->opt.flags & TETSIM_FLAG_REF_GRAB_TEXEL) return fail(h, TETSIM_ESTATE, "body pins on a TETSIM_FLAG_REF_GRAB_TEXEL handle are not supported (its quirk picks other particles, in host arithmetic)");
    if (h->grab_global >= 0) return fail(h, TETSIM_ESTATE, "a handle grab is set (tetsim_set_grab): one kind of hold at a time -- release it first (id -1)");
    if (h->body_grabs_on) return fail(h, TETSIM_ESTATE, kBodyGrabsOn);
    return 0;
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_set_body_pins(tetsim_handle h, const int32_t* particles, const float* targets, uint32_t per_body) {
    if (!h) return TETSIM_EINVAL;
    HIPCHK(h, hipSetDevice(h->opt.device));
    if (!particles) {   // OFF: host state; the table goes back to empty (one that was never made holds nothing)
        h->body_pins_on = false;
        return h->d_pin_rows ? launch_empty_table(h) : 0;
    }
    if (!targets) return fail(h, TETSIM_EINVAL, "targets is null");
    if (int rc = check_per_body(h, per_body)) return rc;
    if (int rc = check_pin_state(h)) return rc;
    const uint32_t nb = num_bodies(h);
    std::vector<uint32_t> first_vert, first_tet;
    body_ranges(h, &first_vert, &first_tet);
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t k = 0; k < per_body; k++) {
            const size_t r = static_cast<size_t>(b) * per_body + k;
            const int32_t p = particles[r];
            const float* t = targets + 3u * r;
            if (p == -1) continue;
            const std::string at = "body " + std::to_string(b) + ", row " + std::to_string(k) + ": ";
            if (p < 0 || static_cast<uint32_t>(p) >= first_vert[b + 1u] - first_vert[b]) return fail(h, TETSIM_EINVAL, at + "particle index outside the body (-1 = unused)");
            if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2])) return fail(h, TETSIM_EINVAL, at + "non-finite target");
        }
    // the winning row of every particle, by the one statement of the rule; the rows that win, translated
    std::vector<uint32_t> counts(nb);
    for (uint32_t b = 0; b < nb; b++) counts[b] = first_vert[b + 1u] - first_vert[b];
    std::vector<int32_t> slot(h->info.num_particles);
    if (tetsim_prep_pin_slots(particles, targets, nb, per_body, counts.data(), slot.data()) != 0) return fail(h, TETSIM_EINVAL, "invalid table");
    std::vector<int4> rows(static_cast<size_t>(nb) * per_body, no_row());
    for (uint32_t a = 0; a < slot.size(); a++) {
        if (slot[a] < 0) continue;
        int4 r;
        r.x = static_cast<int32_t>(h->api2dev.empty() ? a : h->api2dev[a]);
        std::memcpy(&r.y, targets + 3ull * static_cast<uint32_t>(slot[a]), 3 * sizeof(float));
        rows[static_cast<uint32_t>(slot[a])] = r;
    }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_pin_table(h, per_body)) return rc;
    launch_clear(h, nullptr);
    const int rc = launch_row_chunks<Chunk>(h, rows.data(), static_cast<uint32_t>(rows.size()), 1u, [&](const Chunk& c, uint32_t first, uint32_t count) {
        hipLaunchKernelGGL(pin_rows_value_kernel, dim3(1), dim3(kRowsPerLaunch), 0, h->stream, c, h->d_pin_rows, h->d_pin_slot, first, count);
    });
    if (rc) return rc;
    h->body_pins_on = true;
    return 0;
}

int tetsim_set_body_pins_device(tetsim_handle h, const void* particles, const void* targets, uint64_t target_stride, uint32_t per_body, const void* body_mask,
                                void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!particles) {
        if (int rc = device_call_guard(h)) return rc;
        return tetsim_set_body_pins(h, nullptr, nullptr, 0u);
    }
    if (!targets) return fail(h, TETSIM_EINVAL, "targets is null");
    if (int rc = check_per_body(h, per_body)) return rc;
    const uint32_t nb = num_bodies(h), total = nb * per_body;
    return set_rows_device(
        h, [&] { return check_pin_state(h); }, {{particles, "particles", total, 4u, 4u, 0u, nullptr}, {targets, "targets", total, 12u, 4u, target_stride, "target_stride"}},
        body_mask, caller_stream, [&] { return ensure_pin_table(h, per_body); },
        [&] {
            const auto* const p = static_cast<const int32_t*>(particles);
            const auto* const t = static_cast<const char*>(targets);
            const auto* const mask = static_cast<const uint8_t*>(body_mask);
            const uint64_t stride = resolved_stride(target_stride, 12u);
            launch_clear(h, mask);
            hipLaunchKernelGGL(pin_scatter_kernel, dim3(blocks_of(total)), dim3(256), 0, h->stream, p, t, stride, mask, h->d_body_first, h->d_api2dev, h->d_pin_slot, per_body, total);
            hipLaunchKernelGGL(pin_rows_kernel, dim3(blocks_of(total)), dim3(256), 0, h->stream, p, t, stride, mask, h->d_body_first, h->d_api2dev, h->d_pin_slot, h->d_pin_rows,
                               per_body, total);
            return launched(h);
        },
        &h->body_pins_on);
}

}  // extern "C"
