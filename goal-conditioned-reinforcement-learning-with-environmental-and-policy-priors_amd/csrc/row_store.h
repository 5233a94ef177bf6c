// row_store.h -- the aligned row store of the chunked kernels (minigrid_obs.hip, minigrid_render.hip), written once.
//
// A row of F elements at `base` leaves as 16-byte chunks of E elements (16 for bytes, 4 for 32-bit values), counted
// from the 16-byte-aligned address at or below the row's first element: chunk c covers the row positions
// [E * c - s, E * c - s + E), s = the base's misalignment in elements.  A chunk that lies inside the row is one aligned
// 16-byte store; the first and last chunk store only their own elements, one by one.  The arithmetic is plain C++
// (a host compiler takes this file too: tests/test_row_store_cpu.py); the store routine needs hipcc.
#ifndef TWOARMY_ROW_STORE_H
#define TWOARMY_ROW_STORE_H
#include <stdint.h>

#ifdef __HIPCC__
#define MG_ROW_FN __host__ __device__ static inline
#else
#define MG_ROW_FN static inline
#endif

// Elements between `base` (element-aligned) and the 16-byte-aligned address at or below it: 0 .. E - 1.
MG_ROW_FN int mg_row_misalign(const void *base, int E) { return (int)(((uintptr_t)base & 15) * E >> 4); }

// Chunks that cover a row of F elements at misalignment s; for any base (s = E - 1, what a launch must provide).
template <typename I> MG_ROW_FN I mg_row_chunks_at(int s, I F, int E) { return (s + F + E - 1) / E; }
template <typename I> MG_ROW_FN I mg_row_chunks(I F, int E) { return mg_row_chunks_at<I>(E - 1, F, E); }

// Chunk c: its first position p (base + p is 16-byte aligned, p > -E), its own elements [lo, hi) of the row (empty
// for a chunk past the row's end) and whether it is whole, i.e. lies inside the row.
template <typename I> struct mg_row_chunk_t { I p, lo, hi; bool whole; };
template <typename I> MG_ROW_FN mg_row_chunk_t<I> mg_row_chunk(int s, I F, I c, int E)
{
    const I p = E * c - s;
    return {p, p < 0 ? 0 : p, p + E < F ? p + E : F, p >= 0 && p + E <= F};
}

// A workgroup that owns the G chunks from b * G: its chunks [c0, c1) (none if c0 >= c1) and row positions [p_lo, p_hi).
template <typename I> struct mg_row_span_t { I c0, c1, p_lo, p_hi; };
template <typename I> MG_ROW_FN mg_row_span_t<I> mg_row_span(int s, I F, I b, I G, int E)
{
    const I total = mg_row_chunks_at<I>(s, F, E), c0 = b * G, c1 = c0 + G < total ? c0 + G : total;
    return {c0, c1, E * c0 - s < 0 ? 0 : E * c0 - s, E * c1 - s < F ? E * c1 - s : F};
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

// Store chunk c of the row: whole(p) -> the uint4 of elements p .. p + E - 1, one(q) -> element q.
template <typename T, typename I, typename Whole, typename One>
__device__ __forceinline__ void mg_row_store(T *base, I F, I c, Whole whole, One one)
{
    constexpr int E = 16 / sizeof(T);
    const mg_row_chunk_t<I> k = mg_row_chunk<I>(mg_row_misalign(base, E), F, c, E);
    if (k.whole) *reinterpret_cast<uint4 *>(base + k.p) = whole(k.p);
    else for (I q = k.lo; q < k.hi; q++) base[q] = one(q);
}

// The same with the whole chunk built from one(): for values generated in registers.
template <typename T, typename I, typename One>
__device__ __forceinline__ void mg_row_store(T *base, I F, I c, One one)
{
    constexpr int E = 16 / sizeof(T);
    mg_row_store(base, F, c, [&](I p) {
        union { T v[E]; uint4 u; } w;
#pragma unroll
        for (int d = 0; d < E; d++) w.v[d] = one(p + d);
        return w.u;
    }, one);
}
#endif

#endif  // TWOARMY_ROW_STORE_H
