// leafsort_kernels.hpp -- the leaves of a forest sorted tree by tree in digest order (include/vkmr_hip.h:
// vkmr_hip_forest_sort_leaves_async, vkmr_hip_tree_sort_leaves_async; the key, the elements, the ties and the scratch layout:
// leafsort_plan.hpp).  No hash is computed here.
//   *_leafsort_keys_kernel    one lane per element: the key (tree on top, the digest's first words below) and the element's
//                             number as payload; the all-ones sentinel behind the last leaf
//   sort_histogram_kernel, sort_scan_kernel, sort_scatter_kernel   sort_kernels.hpp's passes as they are
//   *_leafsort_ties_kernel    one lane per sorted position: m, the positions whose key equals a neighbour's, by ballots and
//                             one add per workgroup
//   *_leafsort_place_kernel   one lane per sorted position: dest = j, or for a tied position its place in its run of equal
//                             keys by all 256 bits; refuses above VKMR_LEAFSORT_MAX_TIES; counts the leaves equal to an earlier one
//   *_leafsort_emit_kernel    one lane per sorted position: the digest and its input cell written at dest; lane 0 writes info
// Every kernel behind the check reads the status first and follows no offset when it is nonzero.  No kernel waits for another
// workgroup: the order between the phases is that of the launches; the atomics only count.
//
// A forest and one tree differ in where the leaves lie and how a cell finds its tree: the two structs below, in entries.hpp's
// manner -- one body per kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "absence_plan.hpp"
#include "leafsort_plan.hpp"

// Leaves at cells [offsets[0], offsets[ntrees]); the offsets were checked (forest_check_kernel) before any of this is called.
struct LeafsortForest {
    const uint64_t* offsets; uint32_t ntrees;
    __device__ __forceinline__ uint64_t lo() const { return offsets[0]; }
    __device__ __forceinline__ uint64_t n() const { return offsets[ntrees] - offsets[0]; }
    // lo() <= cell < offsets[ntrees]: the upper bound of the cell in offsets[1 .. ntrees], minus one (SortForest::emit's
    // search); an empty tree has an empty range and is never named.
    __device__ __forceinline__ uint32_t tree_of(uint64_t cell) const
    {
        uint32_t a = 1u, b = ntrees;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2u;
            if (offsets[mid] > cell) b = mid;
            else a = mid + 1u;
        }
        return a - 1u;
    }
};

// One tree of `count` leaves at cell 0.
struct LeafsortTree {
    uint64_t count;
    __device__ __forceinline__ uint64_t lo() const { return 0ull; }
    __device__ __forceinline__ uint64_t n() const { return count; }
    __device__ __forceinline__ uint32_t tree_of(uint64_t) const { return 0u; }
};

// `flag` counted over the workgroup into *counter: a ballot per wavefront, an LDS add for counting only, and one global
// atomic per workgroup at the most.  Every lane of the workgroup is here.
__device__ __forceinline__ void leafsort_count(bool flag, unsigned long long* __restrict__ counter)
{
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0u) s_count = 0u;
    __syncthreads();
    const uint64_t set = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u && set) (void)atomicAdd(&s_count, (uint32_t)__popcll(set));
    __syncthreads();
    if (threadIdx.x == 0u && s_count) (void)atomicAdd(counter, (unsigned long long)s_count);
}

// One lane per element i < total: 8 bytes of the leaf are read.
template <class Leaves>
__device__ __forceinline__ void leafsort_keys(const Leaves f, const Node* __restrict__ in, uint32_t total, uint32_t P, const uint64_t* __restrict__ hdr,
                                              uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    uint64_t key = vkmr_leafsort::SENTINEL;
    if (hdr[0] == 0ull && i < f.n()) {
        const uint64_t cell = f.lo() + i;
        const uint2 w = *reinterpret_cast<const uint2*>(in + cell);
        key = vkmr_leafsort::key(f.tree_of(cell), w.x, w.y, P);
    }
    key_out[i] = key;
    val_out[i] = (uint32_t)i;
}

// Sorted position j < n ties when its key is that of j - 1 or of j + 1 < n; the sentinels behind n are not looked at.
__device__ __forceinline__ bool leafsort_tied(const uint64_t* __restrict__ keys, uint64_t j, uint64_t n, uint64_t key)
{
    return (j > 0ull && keys[j - 1ull] == key) || (j + 1ull < n && keys[j + 1ull] == key);
}

// One lane per sorted position: hdr[1] += the positions that tie.  The host zeroed it.
template <class Leaves>
__device__ __forceinline__ void leafsort_ties(const Leaves f, const uint64_t* __restrict__ keys, unsigned long long* __restrict__ hdr)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (hdr[0] != 0ull) return;                          // the same word in every lane
    const uint64_t n = f.n();
    leafsort_count(j < n && leafsort_tied(keys, j, n, keys[j < n ? j : 0ull]), hdr + 1);
}

// One lane per sorted position.  Above the limit nothing is placed and hdr[3] says so (one plain store; no lane of this launch
// reads it).  A tied lane walks its run in both directions from its own position: the loop is as long as the run, which is
// no longer than m <= VKMR_LEAFSORT_MAX_TIES, and neighbouring lanes of a run load the same leaves.
template <class Leaves>
__device__ __forceinline__ void leafsort_place(const Leaves f, const Node* __restrict__ in, const uint64_t* __restrict__ keys,
                                               const uint32_t* __restrict__ src, unsigned long long* __restrict__ hdr, uint32_t* __restrict__ dest)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (hdr[0] != 0ull) return;
    if (hdr[1] > (unsigned long long)VKMR_LEAFSORT_MAX_TIES) {
        if (j == 0ull) hdr[3] = VKMR_LEAFSORT_TOO_MANY_TIES;
        return;
    }
    const uint64_t n = f.n();
    bool repeat = false;
    if (j < n) {
        const uint64_t key = keys[j];
        uint32_t d = (uint32_t)j;
        if (leafsort_tied(keys, j, n, key)) {
            const Node* leaves = in + f.lo();
            const Node me = vkmr_dev::load_node(leaves + src[j]);
            for (uint64_t r = j; r > 0ull && keys[r - 1ull] == key; --r) {        // the earlier members: those above me go behind me
                const Node other = vkmr_dev::load_node(leaves + src[r - 1ull]);
                if (vkmr_absence::less(me.w, other.w)) --d;
                else if (vkmr_dev::node_diff(me, other) == 0u) repeat = true;
            }
            for (uint64_t r = j + 1ull; r < n && keys[r] == key; ++r)               // the later members: those below me go in front
                if (vkmr_absence::less(vkmr_dev::load_node(leaves + src[r]).w, me.w)) ++d;
        }
        dest[j] = d;
    }
    leafsort_count(repeat, hdr + 2);
}

// One lane per sorted position: out[lo + dest[j]] = in[lo + src[j]], and the input cell beside it.  Lane 0 of the launch
// writes info: the status, n (0 when the offsets are bad), m and the repeats (0 unless bits 0 and 1 are clear).
template <class Leaves>
__device__ __forceinline__ void leafsort_emit(const Leaves f, const Node* __restrict__ in, const uint32_t* __restrict__ src,
                                              const uint32_t* __restrict__ dest, const uint64_t* __restrict__ hdr, Node* __restrict__ out,
                                              uint32_t* __restrict__ order_out, uint64_t* __restrict__ info)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t status = hdr[0] | hdr[3];
    if (j == 0ull) {
        info[0] = status;
        info[1] = (hdr[0] & VKMR_LEAFSORT_BAD_OFFSETS) ? 0ull : f.n();
        info[2] = hdr[1];
        info[3] = hdr[2];
    }
    if (status != 0ull || j >= f.n()) return;
    const uint64_t lo = f.lo(), from = lo + src[j], to = lo + dest[j];
    vkmr_dev::store_node(out + to, vkmr_dev::load_node(in + from));
    if (order_out) order_out[to] = (uint32_t)from;
}

__global__ __launch_bounds__(256) void forest_leafsort_keys_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const Node* __restrict__ in,
                                                                   uint32_t total, uint32_t P, const uint64_t* __restrict__ hdr,
                                                                   uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out)
{
    leafsort_keys(LeafsortForest{offsets, ntrees}, in, total, P, hdr, key_out, val_out);
}

__global__ __launch_bounds__(256) void tree_leafsort_keys_kernel(uint64_t count, const Node* __restrict__ in, uint32_t total, uint32_t P,
                                                                 const uint64_t* __restrict__ hdr, uint64_t* __restrict__ key_out,
                                                                 uint32_t* __restrict__ val_out)
{
    leafsort_keys(LeafsortTree{count}, in, total, P, hdr, key_out, val_out);
}

__global__ __launch_bounds__(256) void forest_leafsort_ties_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const uint64_t* __restrict__ keys,
                                                                   unsigned long long* __restrict__ hdr)
{
    leafsort_ties(LeafsortForest{offsets, ntrees}, keys, hdr);
}

__global__ __launch_bounds__(256) void tree_leafsort_ties_kernel(uint64_t count, const uint64_t* __restrict__ keys, unsigned long long* __restrict__ hdr)
{
    leafsort_ties(LeafsortTree{count}, keys, hdr);
}

__global__ __launch_bounds__(256) void forest_leafsort_place_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const Node* __restrict__ in,
                                                                    const uint64_t* __restrict__ keys, const uint32_t* __restrict__ src,
                                                                    unsigned long long* __restrict__ hdr, uint32_t* __restrict__ dest)
{
    leafsort_place(LeafsortForest{offsets, ntrees}, in, keys, src, hdr, dest);
}

__global__ __launch_bounds__(256) void tree_leafsort_place_kernel(uint64_t count, const Node* __restrict__ in, const uint64_t* __restrict__ keys,
                                                                  const uint32_t* __restrict__ src, unsigned long long* __restrict__ hdr,
                                                                  uint32_t* __restrict__ dest)
{
    leafsort_place(LeafsortTree{count}, in, keys, src, hdr, dest);
}

__global__ __launch_bounds__(256) void forest_leafsort_emit_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const Node* __restrict__ in,
                                                                   const uint32_t* __restrict__ src, const uint32_t* __restrict__ dest,
                                                                   const uint64_t* __restrict__ hdr, Node* __restrict__ out,
                                                                   uint32_t* __restrict__ order_out, uint64_t* __restrict__ info)
{
    leafsort_emit(LeafsortForest{offsets, ntrees}, in, src, dest, hdr, out, order_out, info);
}

__global__ __launch_bounds__(256) void tree_leafsort_emit_kernel(uint64_t count, const Node* __restrict__ in, const uint32_t* __restrict__ src,
                                                                 const uint32_t* __restrict__ dest, const uint64_t* __restrict__ hdr,
                                                                 Node* __restrict__ out, uint32_t* __restrict__ order_out, uint64_t* __restrict__ info)
{
    leafsort_emit(LeafsortTree{count}, in, src, dest, hdr, out, order_out, info);
}
