// merge_kernels.hpp -- two sorted forests merged tree by tree: union, difference, intersection (include/vkmr_hip.h:
// vkmr_hip_forest_merge_leaves_async, vkmr_hip_tree_merge_leaves_async; the slots, the placement and the scratch layout:
// merge_plan.hpp).  No hash is computed here.
//   forest_check_kernel       forest_kernels.hpp's, once for A's offsets and once for B's, each into a header word of its own
//   *_merge_order_kernel      one lane per element of A: its cell against the one in front; only an offending lane looks for its
//                             tree (a pair that straddles two trees is no offence) and sets status bit 2
//   *_merge_mark_kernel       one lane per element of B: its tree, its predecessor (bit 3, the repeats), the lower bound in A_t
//                             by absence_plan.hpp's loop, the match; then the count or the mark at its slot, its flag and pos0
//   sort_scan_kernel          sort_kernels.hpp's, as it is, twice: the rows of the slots and flags, then the row sums
//   *_merge_emit_kernel       one lane per element of A and, for union, of B: one 32-byte load and one 32-byte store to the
//                             closed-form cell, the origin beside it; the first ntrees + 1 lanes write out_offsets, lane 0 info
// The order and mark kernels read the offsets checks first and follow no offset when one failed; the emit kernel forms the whole
// status, bit 4 included, before it writes a cell.  No kernel waits for another workgroup: the order between the phases is that
// of the launches; the atomics only count (and OR status bits).
//
// A forest and one tree differ in where the leaves lie and how a cell finds its tree: the two structs below, in entries.hpp's
// manner -- one body per kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "absence_kernels.hpp"   // absence_bound
#include "merge_plan.hpp"

// A at cells [a_offsets[0], a_offsets[ntrees]) and B likewise; the offsets were checked before any of this is called.
struct MergeForest {
    static constexpr bool forest = true;
    const uint64_t* a_offsets; const uint64_t* b_offsets; uint32_t ntrees;
    __device__ __forceinline__ uint32_t trees() const { return ntrees; }
    __device__ __forceinline__ uint64_t a_lo() const { return a_offsets[0]; }
    __device__ __forceinline__ uint64_t a_n() const { return a_offsets[ntrees] - a_offsets[0]; }
    __device__ __forceinline__ uint64_t b_lo() const { return b_offsets[0]; }
    __device__ __forceinline__ uint64_t b_n() const { return b_offsets[ntrees] - b_offsets[0]; }
    __device__ __forceinline__ uint64_t a_first(uint32_t t) const { return a_offsets[t]; }    // t <= ntrees
    __device__ __forceinline__ uint64_t b_first(uint32_t t) const { return b_offsets[t]; }
    // offsets[0] <= cell < offsets[ntrees]: the upper bound of the cell in offsets[1 .. ntrees], minus one (LeafsortForest's).
    static __device__ __forceinline__ uint32_t tree_of(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t cell)
    {
        uint32_t a = 1u, b = ntrees;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2u;
            if (offsets[mid] > cell) b = mid;
            else a = mid + 1u;
        }
        return a - 1u;
    }
    __device__ __forceinline__ uint32_t a_tree(uint64_t cell) const { return tree_of(a_offsets, ntrees, cell); }
    __device__ __forceinline__ uint32_t b_tree(uint64_t cell) const { return tree_of(b_offsets, ntrees, cell); }
};

// One tree of a_count leaves against one of b_count, both at cell 0.
struct MergeTree {
    static constexpr bool forest = false;
    uint64_t a_count, b_count;
    __device__ __forceinline__ uint32_t trees() const { return 1u; }
    __device__ __forceinline__ uint64_t a_lo() const { return 0ull; }
    __device__ __forceinline__ uint64_t a_n() const { return a_count; }
    __device__ __forceinline__ uint64_t b_lo() const { return 0ull; }
    __device__ __forceinline__ uint64_t b_n() const { return b_count; }
    __device__ __forceinline__ uint64_t a_first(uint32_t t) const { return t ? a_count : 0ull; }
    __device__ __forceinline__ uint64_t b_first(uint32_t t) const { return t ? b_count : 0ull; }
    __device__ __forceinline__ uint32_t a_tree(uint64_t) const { return 0u; }
    __device__ __forceinline__ uint32_t b_tree(uint64_t) const { return 0u; }
};

// The offsets checks of both sides as status bits 0 and 1 (one tree has none: the words stay zero).
__device__ __forceinline__ uint64_t merge_offsets_status(const unsigned long long* __restrict__ hdr)
{
    return (hdr[3] ? VKMR_MERGE_BAD_A_OFFSETS : 0ull) | (hdr[4] ? VKMR_MERGE_BAD_B_OFFSETS : 0ull);
}

// One lane per element i < a_total of A.
template <class Leaves>
__device__ __forceinline__ void merge_order(const Leaves f, const Node* __restrict__ a, unsigned long long* __restrict__ hdr)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (merge_offsets_status(hdr) != 0ull) return;
    if (i == 0ull || i >= f.a_n()) return;
    const uint64_t cell = f.a_lo() + i;
    if (vkmr_absence::less(vkmr_dev::load_node(a + cell - 1ull).w, vkmr_dev::load_node(a + cell).w)) return;
    if (f.a_first(f.a_tree(cell)) == cell) return;         // the first leaf of its tree
    (void)atomicOr(hdr, (unsigned long long)VKMR_MERGE_A_NOT_INCREASING);
}

// `first` and `second` counted over the workgroup into counter[0] and counter[1]: a ballot per wavefront, LDS adds for counting
// only, and one global atomic per counter and workgroup at the most.  Every lane of the workgroup is here.
__device__ __forceinline__ void merge_count(bool first, bool second, unsigned long long* __restrict__ counter)
{
    __shared__ uint32_t s_count[2];
    if (threadIdx.x < 2u) s_count[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t one = __ballot(first), two = __ballot(second);
    if ((threadIdx.x & 63u) == 0u) {
        if (one) (void)atomicAdd(&s_count[0], (uint32_t)__popcll(one));
        if (two) (void)atomicAdd(&s_count[1], (uint32_t)__popcll(two));
    }
    __syncthreads();
    if (threadIdx.x < 2u && s_count[threadIdx.x]) (void)atomicAdd(counter + threadIdx.x, (unsigned long long)s_count[threadIdx.x]);
}

// One lane per element j < b_total of B.  scan: the zeroed slots and flags; S: where the flags begin.
template <class Leaves>
__device__ __forceinline__ void merge_mark(const Leaves f, const Node* __restrict__ a, const Node* __restrict__ b, uint32_t op, uint64_t S,
                                           unsigned long long* __restrict__ hdr, uint32_t* __restrict__ scan, uint32_t* __restrict__ pos0)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (merge_offsets_status(hdr) != 0ull) return;         // the same words in every lane
    bool repeat = false, match = false;
    if (j < f.b_n()) {
        const uint64_t cell = f.b_lo() + j;
        const uint32_t t = f.b_tree(cell);
        const Node me = vkmr_dev::load_node(b + cell);
        if (cell > f.b_first(t)) {
            const Node before = vkmr_dev::load_node(b + cell - 1ull);
            if (vkmr_absence::less(me.w, before.w)) (void)atomicOr(hdr, (unsigned long long)VKMR_MERGE_B_DECREASES);
            repeat = vkmr_dev::node_diff(me, before) == 0u;
        }
        const uint64_t o = f.a_first(t), c = f.a_first(t + 1u) - o;
        const uint64_t lb = absence_bound(a + o, c, me);
        match = lb < c && vkmr_dev::node_diff(vkmr_dev::load_node(a + o + lb), me) == 0u;
        const uint64_t slot = o - f.a_lo() + lb;
        const bool keep = vkmr_merge::kept(op, repeat, match);
        if (keep) {
            (void)atomicAdd(scan + slot, 1u);
            scan[S + j] = 1u;
        }
        if (vkmr_merge::marks(op, repeat, match)) scan[slot] = 1u;
        pos0[j] = keep ? (uint32_t)slot : VKMR_MERGE_NONE;
        match = match && !repeat;
    }
    merge_count(match, repeat, hdr + 1);
}

// One lane per element of A, then (union) per element of B; the first trees() + 1 lanes write the offsets as well.
template <class Leaves>
__device__ __forceinline__ void merge_emit(const Leaves f, const Node* __restrict__ a, const Node* __restrict__ b, uint32_t op, uint64_t a_total,
                                           uint64_t b_total, const unsigned long long* __restrict__ hdr, const uint32_t* __restrict__ row,
                                           const uint32_t* __restrict__ tot, const uint32_t* __restrict__ pos0, uint64_t out_capacity,
                                           Node* __restrict__ out, uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ origin,
                                           uint64_t* __restrict__ info)
{
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t status = merge_offsets_status(hdr) | hdr[0];
    if (status != 0ull) {
        if (x == 0ull) { info[0] = status; info[1] = 0ull; info[2] = 0ull; info[3] = 0ull; }
        return;
    }
    const uint64_t S = vkmr_merge::slots(a_total), nA = f.a_n(), nB = f.b_n();
    const uint32_t e_S = vkmr_merge::prefix(row, tot, S);
    const uint64_t n_out = vkmr_merge::n_out(op, nA, e_S);
    if (n_out > out_capacity) status = VKMR_MERGE_SHORT_OUTPUT;
    if (x == 0ull) { info[0] = status; info[1] = n_out; info[2] = hdr[1]; info[3] = hdr[2]; }
    if (status != 0ull) return;
    if constexpr (Leaves::forest) {
        if (x <= (uint64_t)f.trees()) {
            const uint32_t t = (uint32_t)x;
            const uint64_t base_a = f.a_first(t) - f.a_lo(), base_b = f.b_first(t) - f.b_lo();
            out_offsets[t] = vkmr_merge::tree_start(op, base_a, vkmr_merge::prefix(row, tot, base_a), vkmr_merge::prefix(row, tot, S + base_b) - e_S);
        }
    }
    if (x < a_total) {
        uint64_t dest;
        if (x < nA && vkmr_merge::a_dest(op, x, vkmr_merge::prefix(row, tot, x), vkmr_merge::prefix(row, tot, x + 1ull), &dest)) {
            const uint64_t from = f.a_lo() + x;
            vkmr_dev::store_node(out + dest, vkmr_dev::load_node(a + from));
            if (origin) origin[dest] = from;
        }
        return;
    }
    const uint64_t j = x - a_total;
    if (op != VKMR_MERGE_UNION || j >= b_total || j >= nB) return;
    const uint32_t p = pos0[j];
    if (p == VKMR_MERGE_NONE) return;
    const uint64_t from = f.b_lo() + j, dest = vkmr_merge::b_dest(p, vkmr_merge::prefix(row, tot, S + j) - e_S);
    vkmr_dev::store_node(out + dest, vkmr_dev::load_node(b + from));
    if (origin) origin[dest] = from | VKMR_MERGE_ORIGIN_B;
}

__global__ __launch_bounds__(256) void forest_merge_order_kernel(const uint64_t* __restrict__ a_offsets, const uint64_t* __restrict__ b_offsets,
                                                                 uint32_t ntrees, const Node* __restrict__ a, unsigned long long* __restrict__ hdr)
{
    merge_order(MergeForest{a_offsets, b_offsets, ntrees}, a, hdr);
}

__global__ __launch_bounds__(256) void tree_merge_order_kernel(uint64_t a_count, uint64_t b_count, const Node* __restrict__ a,
                                                               unsigned long long* __restrict__ hdr)
{
    merge_order(MergeTree{a_count, b_count}, a, hdr);
}

__global__ __launch_bounds__(256) void forest_merge_mark_kernel(const uint64_t* __restrict__ a_offsets, const uint64_t* __restrict__ b_offsets,
                                                                uint32_t ntrees, const Node* __restrict__ a, const Node* __restrict__ b, uint32_t op,
                                                                uint64_t S, unsigned long long* __restrict__ hdr, uint32_t* __restrict__ scan,
                                                                uint32_t* __restrict__ pos0)
{
    merge_mark(MergeForest{a_offsets, b_offsets, ntrees}, a, b, op, S, hdr, scan, pos0);
}

__global__ __launch_bounds__(256) void tree_merge_mark_kernel(uint64_t a_count, uint64_t b_count, const Node* __restrict__ a, const Node* __restrict__ b,
                                                              uint32_t op, uint64_t S, unsigned long long* __restrict__ hdr, uint32_t* __restrict__ scan,
                                                              uint32_t* __restrict__ pos0)
{
    merge_mark(MergeTree{a_count, b_count}, a, b, op, S, hdr, scan, pos0);
}

__global__ __launch_bounds__(256) void forest_merge_emit_kernel(const uint64_t* __restrict__ a_offsets, const uint64_t* __restrict__ b_offsets,
                                                                uint32_t ntrees, const Node* __restrict__ a, const Node* __restrict__ b, uint32_t op,
                                                                uint64_t a_total, uint64_t b_total, const unsigned long long* __restrict__ hdr,
                                                                const uint32_t* __restrict__ row, const uint32_t* __restrict__ tot,
                                                                const uint32_t* __restrict__ pos0, uint64_t out_capacity, Node* __restrict__ out,
                                                                uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ origin,
                                                                uint64_t* __restrict__ info)
{
    merge_emit(MergeForest{a_offsets, b_offsets, ntrees}, a, b, op, a_total, b_total, hdr, row, tot, pos0, out_capacity, out, out_offsets, origin, info);
}

__global__ __launch_bounds__(256) void tree_merge_emit_kernel(uint64_t a_count, uint64_t b_count, const Node* __restrict__ a, const Node* __restrict__ b,
                                                              uint32_t op, const unsigned long long* __restrict__ hdr, const uint32_t* __restrict__ row,
                                                              const uint32_t* __restrict__ tot, const uint32_t* __restrict__ pos0, uint64_t out_capacity,
                                                              Node* __restrict__ out, uint64_t* __restrict__ origin, uint64_t* __restrict__ info)
{
    merge_emit(MergeTree{a_count, b_count}, a, b, op, a_count, b_count, hdr, row, tot, pos0, out_capacity, out, (uint64_t*)nullptr, origin, info);
}
