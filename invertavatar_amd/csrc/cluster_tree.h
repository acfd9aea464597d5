// The implicit cluster tree over the triangles of a mesh and the wave-union walk over it, shared by the queries on the tree
// (winding_tree.hip; closest_tree.hip, 4.23).  Like geom_common.h: inline functions and templates, no kernels; the walk
// is a macro body, which leaves the two query kernels' device code as it was.  geometry._tree_walk restates it in NumPy.
//
// Tree     : leaf i = sorted faces [i L, min((i + 1) L, Fu)), L = kLeaf (the Morton order is winding_tree.hip's); level k + 1 groups
//            B = kBranch consecutive nodes of level k until one root is left.  Node (level, index) sits at row start[level] + index of
//            every per-node table, leaves first; there are no pointers.
// Walk     : per point depth first from the root, children in index order.  A wave walks the UNION of its 64 lanes' traversals
//            without a stack: (l, j) are wave-uniform, what is below a node is entered while the ballot of lanes that need it is
//            non-zero, and a lane that accepted a node (winding: far; closest point: skipped) stays masked until the walk leaves that
//            subtree.  Rows and leaf triangles are wave-uniform loads: every lane executes every visit of the union, uses only what
//            it needs and adds its own terms in its own order, so its result does not depend on which points share its wave.
#pragma once

#include "geom_common.h"

namespace ia {
namespace tree {

constexpr int kLeaf = 32;                            // faces per leaf: part of the results
constexpr int kBranch = 8;                           // children per upper node: part of the results
constexpr int kLeafShift = 5, kBranchShift = 3;
constexpr int kMaxLevels = 8;                        // 2^25 faces -> 2^20 leaves -> 8 levels
constexpr int64_t kMaxFaces = (int64_t)1 << 25;      // the limit of ia_tri_pack
static_assert((1 << kLeafShift) == kLeaf && (1 << kBranchShift) == kBranch, "shifts");

struct Levels {
    int n;                                           // number of levels (0: no usable face)
    int count[kMaxLevels];
    int start[kMaxLevels];
    int total;
};
inline Levels levels_of(int64_t Fu) {
    Levels t = {};
    if (Fu <= 0) return t;
    int64_t c = ceil_div(Fu, (int64_t)kLeaf);
    for (;;) {
        t.count[t.n] = (int)c;
        t.start[t.n] = t.total;
        t.total += (int)c;
        ++t.n;
        if (c == 1) break;
        c = ceil_div(c, (int64_t)kBranch);
    }
    return t;
}

struct Tree {                                        // what a kernel is given
    int top;                                         // level of the root; -1: no node
    int start[kMaxLevels];
};
inline Tree tree_of(const Levels& t) {
    Tree tree = {};
    tree.top = t.n - 1;
    for (int l = 0; l < t.n; ++l) tree.start[l] = t.start[l];
    return tree;
}

// The argument checks of the entry points; `what`: the entry point's name.
inline int check_faces(int64_t Fu, const char* what) {
    return Fu >= 0 && Fu <= kMaxFaces ? IA_OK : fail(IA_ERR_INVALID_ARG, "%s: F_usable must be >= 0 and <= 2^25, got %lld", what, (long long)Fu);
}
inline int check_points(int64_t N, const char* what) {
    return N >= 0 && N < ((int64_t)1 << 31) / 3 ? IA_OK : fail(IA_ERR_INVALID_ARG, "%s: N must be >= 0 and 3 N < 2^31, got %lld", what, (long long)N);
}
inline int check_nodes(const Levels& t, int64_t Fu, int64_t n, const char* what) {
    return n == t.total ? IA_OK : fail(IA_ERR_INVALID_ARG, "%s: %lld usable faces make %d nodes, got n_nodes = %lld", what, (long long)Fu, t.total, (long long)n);
}
struct Range { int lo, hi; };
struct Tri { float4 A, B, C; };                      // a packed triangle (ia_tri_pack)

// Nodes of level l over Fu faces; the sorted faces of leaf i; the children of node j of a level above `children` nodes.
#define IA_TREE_COUNT(Fu, l) (((Fu) + (kLeaf << (kBranchShift * (l))) - 1) >> (kLeafShift + kBranchShift * (l)))
__device__ __forceinline__ int level_count(int Fu, int l) { return IA_TREE_COUNT(Fu, l); }
__device__ __forceinline__ Range leaf_range(int i, int Fu) { return {i * kLeaf, min(i * kLeaf + kLeaf, Fu)}; }
__device__ __forceinline__ Range child_range(int j, int children) { return {j * kBranch, min(j * kBranch + kBranch, children)}; }
__device__ __forceinline__ Vec3<float> xyz(float4 v) { return {v.x, v.y, v.z}; }
__device__ __forceinline__ Tri load_tri(const float4* __restrict__ tris, int f) { return {tris[3 * (int64_t)f], tris[3 * (int64_t)f + 1], tris[3 * (int64_t)f + 2]}; }

}  // namespace tree
}  // namespace ia

// The walk, in a kernel with `using namespace ia::tree`:
//     IA_TREE_STAGE(tree);                          every thread of the workgroup, before anything diverges: s_start[] in LDS, once
//     IA_TREE_WALK(tree, ok)                        ok: this lane walks at all (not past the end, a finite point)
//         ... at node (l, j) = table row `node`.  IA_TREE_WALKING: the lane neither waits under a node nor never walks.  Do the lane's
//         own work and define two bools, each `IA_TREE_WALKING && ...`: `hold` (the lane accepts the node and waits under it) and
//         `need` (it needs what is below).  Whatever else makes a lane pass over a node (closest_tree.hip's seed leaf) belongs here.
//     IA_TREE_LEAF
//         ... the per-face loop of leaf j, in every lane, when some lane needs it; `need` is the lane's own.
//     IA_TREE_END(tree, AHEAD, COUNT)               COUNT: the nodes of level l; AHEAD: a statement in front of the sibling test
// The names above and `held` are the walk's.  Where the count is evaluated is each kernel's own (winding: IA_TREE_COUNT ahead of the
// test; closest point: level_count inside it), as it was before this header: with that, both kernels' device code is unchanged.
#define IA_TREE_WALKING (held < 0)
#define IA_TREE_STAGE(tree)                                                                          \
    __shared__ int s_start[kMaxLevels];                                                              \
    if (threadIdx.x < kMaxLevels) s_start[threadIdx.x] = (tree).start[threadIdx.x];                  \
    __syncthreads()
#define IA_TREE_WALK(tree, ok)                                                                       \
    int held = (ok) ? -1 : kMaxLevels;   /* level of the node this lane waits under; -1: walking; kMaxLevels: never walks */ \
    int l = (tree).top, j = 0;           /* (wave-uniform) */                                        \
    while (l >= 0) {                                                                                 \
        const int node = __builtin_amdgcn_readfirstlane(s_start[l]) + j;
#define IA_TREE_LEAF                                                                                 \
        if (hold) held = l;                                                                          \
        if (l > 0) {                                                                                 \
            if (__ballot(need)) {        /* some lane needs the children */                          \
                --l;                                                                                 \
                j *= kBranch;                                                                        \
                continue;                                                                            \
            }                                                                                        \
        } else if (__ballot(need)) {     /* (the same triangles in every lane) */
#define IA_TREE_END(tree, AHEAD, COUNT)                                                              \
        }                                                                                            \
        for (;;) {                       /* the subtree of (l, j) is done: the next node in depth-first order */ \
            if (held == l) held = -1;                                                                \
            if (l == (tree).top) { l = -1; break; }                                                  \
            AHEAD;                                                                                   \
            if (((j + 1) & (kBranch - 1)) != 0 && j + 1 < (COUNT)) { ++j; break; }                   \
            j >>= kBranchShift;                                                                      \
            ++l;                                                                                     \
        }                                                                                            \
    }
