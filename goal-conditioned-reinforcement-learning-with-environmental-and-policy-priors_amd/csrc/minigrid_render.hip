/*
 * minigrid_render.hip -- device renderer for MiniGrid worlds kept as SoA planes (C ABI: include/minigrid_render.h).
 *
 *   mg_render_atlas_kernel   one workgroup per atlas tile: 3 x 3 supersampled rasterisation in float64, in the
 *                            operation order of the reference's rendering.py / Grid.render_tile, so that the bytes
 *                            are the reference's.  Runs once per tile size.
 *   mg_render_kernel<Cells>  the frame: a gather of atlas bytes selected by the cells the frame shows -- the world's
 *                            (mg_world_cells, mg_render) or the agent's rotated, wall-padded view (mg_view_cells,
 *                            mg_render_pov); the gather itself is written once.  The body of every
 *                            frame leaves as aligned 16-byte stores, its two ends byte by byte.  Its byte budget is
 *                            that of a store stream; measured, the gather's index arithmetic and unaligned fetches
 *                            bound it well below the store rate.
 *   mg_highlight_mask_kernel the highlight loop of get_full_render in gather form (one thread per world cell).
 *
 * Floating point: every expression below is evaluated the way CPython / numpy evaluate the reference's, one IEEE
 * double operation at a time -- contraction into fused multiply-adds is switched off for this file, and cos / sin
 * come from the host's libm (mg_render_constants), never from the device.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "launch.h"
#include "minigrid_render.h"
#include "minigrid_view.h"
#include "row_store.h"
#include "twoarmy.h"
#include "view_map.h"

#pragma clang fp contract(off)

#define MG_RENDER_THREADS 256
#define MG_RENDER_CHUNKS 1024           /* 16-byte chunks per workgroup of mg_render_kernel (16 KiB of frame) */

struct mg_render_consts {
    double cs[4], sn[4];                /* cos / sin of -0.5 * pi * dir */
    double ax, ay, v0x, v0y, v1x, v1y;  /* triangle vertex a, v0 = c - a, v1 = b - a (float32 values) */
    double dot00, dot01, dot11, inv_denom;
};

/* ------------------------------------------------------------------------------------------------ tile index */
__host__ __device__ static inline int mg_tile_index(int type, int colour, int state, int agent_dir, int highlight)
{
    int kind, col = colour;
    switch (type) {
    case 0: case 1: kind = 0; col = 0; break;
    case 2: kind = 1; break;
    case 3: kind = 2; break;
    case 4: kind = state == 0 ? 3 : (state == 2 ? 5 : 4); break;
    case 5: kind = 6; break;
    case 6: kind = 7; break;
    case 7: kind = 8; break;
    case 8: kind = 9; col = 1; break;
    default: return -1;
    }
    if (col < 0 || col > 5) return -1;
    const int av = agent_dir < 0 ? 0 : 1 + (agent_dir & 3);
    return ((kind * 6 + col) * 5 + av) * 2 + (highlight ? 1 : 0);
}

/* ------------------------------------------------------------------------------------------------ rasteriser */
__device__ static inline bool mg_in_rect(double x, double y, double xmin, double xmax, double ymin, double ymax)
{
    return x >= xmin && x <= xmax && y >= ymin && y <= ymax;
}

__device__ static inline bool mg_in_circle(double x, double y, double cx, double cy, double r)
{
    return (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r * r;
}

/* rotate_fn(point_in_triangle((0.12, 0.19), (0.87, 0.50), (0.12, 0.81)), 0.5, 0.5, 0.5 * pi * dir)(x, y) */
__device__ static inline bool mg_in_agent(double x, double y, int dir, const mg_render_consts &k)
{
    const double cx = 0.5, cy = 0.5;
    x = x - cx;
    y = y - cy;
    const double x2 = cx + x * k.cs[dir] - y * k.sn[dir];
    const double y2 = cy + y * k.cs[dir] + x * k.sn[dir];
    const double v2x = x2 - k.ax, v2y = y2 - k.ay;
    const double dot02 = k.v0x * v2x + k.v0y * v2y;
    const double dot12 = k.v1x * v2x + k.v1y * v2y;
    const double u = (k.dot11 * dot02 - k.dot01 * dot12) * k.inv_denom;
    const double v = (k.dot00 * dot12 - k.dot01 * dot02) * k.inv_denom;
    return u >= 0 && v >= 0 && (u + v) < 1;
}

/* One sample of Grid.render_tile's supersampled image before the downsample: sample (sx, sy) of S x S, packed
 * r | g << 8 | b << 16.  The only place the tiles' geometry is written. */
__device__ static uint32_t mg_tile_sample(int kind, int col, int agent_dir, int highlight, int sx, int sy, int S,
                                          const mg_render_consts &k)
{
    const uint32_t COLORS[6] = {0x0000FFu, 0x00FF00u, 0xFF0000u, 0xC32770u, 0x00FFFFu, 0x646464u};
    const uint32_t BLACK = 0, GREY = 0x646464u;
    const double x = (sx + 0.5) / S, y = (sy + 0.5) / S;
    const uint32_t c = COLORS[col];
    uint32_t p = BLACK;
    if (mg_in_rect(x, y, 0, 0.031, 0, 1)) p = GREY;                   /* grid lines: left, then top edge */
    if (mg_in_rect(x, y, 0, 1, 0, 0.031)) p = GREY;
    switch (kind) {
    case 1:                                                           /* Wall */
    case 9:                                                           /* Goal (col = green) */
        if (mg_in_rect(x, y, 0, 1, 0, 1)) p = c;
        break;
    case 2: {                                                         /* Floor: COLORS / 2, truncated on assignment */
        uint32_t h = 0;
        for (int ch = 0; ch < 3; ch++) h |= (uint32_t)(int)((double)((c >> (8 * ch)) & 255u) / 2) << (8 * ch);
        if (mg_in_rect(x, y, 0.031, 1, 0.031, 1)) p = h;
        break;
    }
    case 3:                                                           /* Door, open */
        if (mg_in_rect(x, y, 0.88, 1.00, 0.00, 1.00)) p = c;
        if (mg_in_rect(x, y, 0.92, 0.96, 0.04, 0.96)) p = BLACK;
        break;
    case 4:                                                           /* Door, closed */
        if (mg_in_rect(x, y, 0.00, 1.00, 0.00, 1.00)) p = c;
        if (mg_in_rect(x, y, 0.04, 0.96, 0.04, 0.96)) p = BLACK;
        if (mg_in_rect(x, y, 0.08, 0.92, 0.08, 0.92)) p = c;
        if (mg_in_rect(x, y, 0.12, 0.88, 0.12, 0.88)) p = BLACK;
        if (mg_in_circle(x, y, 0.75, 0.50, 0.08)) p = c;
        break;
    case 5: {                                                         /* Door, locked: 0.45 * colour, truncated */
        uint32_t h = 0;
        for (int ch = 0; ch < 3; ch++) h |= (uint32_t)(int)(0.45 * (double)((c >> (8 * ch)) & 255u)) << (8 * ch);
        if (mg_in_rect(x, y, 0.00, 1.00, 0.00, 1.00)) p = c;
        if (mg_in_rect(x, y, 0.06, 0.94, 0.06, 0.94)) p = h;
        if (mg_in_rect(x, y, 0.52, 0.75, 0.50, 0.56)) p = c;
        break;
    }
    case 6:                                                           /* Key */
        if (mg_in_rect(x, y, 0.50, 0.63, 0.31, 0.88)) p = c;
        if (mg_in_rect(x, y, 0.38, 0.50, 0.59, 0.66)) p = c;
        if (mg_in_rect(x, y, 0.38, 0.50, 0.81, 0.88)) p = c;
        if (mg_in_circle(x, y, 0.56, 0.28, 0.190)) p = c;
        if (mg_in_circle(x, y, 0.56, 0.28, 0.064)) p = BLACK;
        break;
    case 7:                                                           /* Ball */
        if (mg_in_circle(x, y, 0.5, 0.5, 0.31)) p = c;
        break;
    case 8:                                                           /* Box */
        if (mg_in_rect(x, y, 0.12, 0.88, 0.12, 0.88)) p = c;
        if (mg_in_rect(x, y, 0.18, 0.82, 0.18, 0.82)) p = BLACK;
        if (mg_in_rect(x, y, 0.16, 0.84, 0.47, 0.53)) p = c;
        break;
    default:                                                          /* empty */
        break;
    }
    if (agent_dir >= 0 && mg_in_agent(x, y, agent_dir, k)) p = 0x0000FFu;
    if (highlight) {                                                  /* highlight_img: img + 0.3 * (255 - img) */
        uint32_t h = 0;
        for (int ch = 0; ch < 3; ch++) {
            const int v = (int)((p >> (8 * ch)) & 255u);
            double b = (double)v + 0.30 * (double)(255 - v);
            b = b < 0 ? 0 : (b > 255 ? 255 : b);
            h |= (uint32_t)(int)b << (8 * ch);
        }
        p = h;
    }
    return p;
}

/* downsample(img, 3) + the truncating cast of Grid.render's assignment: mean over the three samples of a row
 * (axis 3), then over the three rows (axis 1), each a left-to-right float64 sum divided by 3. */
__global__ __launch_bounds__(MG_RENDER_THREADS) void mg_render_atlas_kernel(int ts, uint8_t *__restrict__ atlas,
                                                                             mg_render_consts k)
{
    const int tile = blockIdx.x;
    const int hl = tile & 1, av = (tile >> 1) % 5, kc = (tile >> 1) / 5, col = kc % 6, kind = kc / 6;
    const int S = 3 * ts;
    uint8_t *out = atlas + (size_t)tile * ts * ts * 3;
    for (int px = threadIdx.x; px < ts * ts; px += MG_RENDER_THREADS) {
        const int oy = px / ts, ox = px - oy * ts;
        double m[3][3];
        for (int dy = 0; dy < 3; dy++) {
            uint32_t s[3];
            for (int dx = 0; dx < 3; dx++) s[dx] = mg_tile_sample(kind, col, av - 1, hl, 3 * ox + dx, 3 * oy + dy, S, k);
            for (int ch = 0; ch < 3; ch++) {
                const double a = (double)((s[0] >> (8 * ch)) & 255u), b = (double)((s[1] >> (8 * ch)) & 255u),
                             c = (double)((s[2] >> (8 * ch)) & 255u);
                m[dy][ch] = ((a + b) + c) / 3.0;
            }
        }
        for (int ch = 0; ch < 3; ch++) out[px * 3 + ch] = (uint8_t)(int)(((m[0][ch] + m[1][ch]) + m[2][ch]) / 3.0);
    }
}

/* ------------------------------------------------------------------------------------------------ frame */
struct mg_cell { int type, colour, state, agent, highlight; };     /* agent: direction, -1 = the agent is not here */

/* The two pictures a frame can show.  A cell source is built per output frame and answers "what does cell
 * cy * W + cx of this frame's W x H cells hold"; the gather below is written against that question alone. */

/* Grid.render of the world itself (mg_render): frame cell = world cell. */
struct mg_world_cells {
    struct args {
        const uint8_t *type, *colour, *state, *highlight;
        const int32_t *agent_x, *agent_y, *agent_dir;
        int astride;
    };
    const uint8_t *ty, *co, *st, *hm;
    int acell, ad;
    __device__ mg_world_cells(const args &a, int e, int W, int H)
    {
        const int HW = W * H;
        ty = a.type + (int64_t)e * HW;
        co = a.colour + (int64_t)e * HW;
        st = a.state ? a.state + (int64_t)e * HW : nullptr;
        hm = a.highlight ? a.highlight + (int64_t)e * HW : nullptr;
        const int ax = a.agent_x[(int64_t)e * a.astride], ay = a.agent_y[(int64_t)e * a.astride];
        ad = a.agent_dir[(int64_t)e * a.astride] & 3;
        acell = (ax >= 0 && ax < W && ay >= 0 && ay < H) ? ay * W + ax : -1;
    }
    __device__ mg_cell at(int cell) const
    {
        return {ty[cell], co[cell], st ? st[cell] : 0, cell == acell ? ad : -1, hm ? hm[cell] != 0 : 0};
    }
};

/* get_pov_render (mg_render_pov): the V x V frame cell (i, j) is the world cell gen_obs_grid puts there (view_map.h),
 * a grey wall outside the world; the highlight is the view's visibility mask, and a cell the mask hides is drawn
 * empty (process_vis clears it in the grid it is handed, minigrid.py:827-830); the agent's own cell (V / 2, V - 1)
 * holds the carried object, placed after process_vis, under the triangle of direction 3. */
struct mg_view_cells {
    struct args {
        const uint8_t *type, *colour, *state, *carrying, *vis_mask;
        const int32_t *agent_x, *agent_y, *agent_dir;
        int astride, width, height;
    };
    const uint8_t *ty, *co, *st, *vm;
    int W, H, V, topx, topy, rot;
    mg_cell carried;
    __device__ mg_view_cells(const args &a, int e, int v, int)
    {
        W = a.width; H = a.height; V = v;
        const int HW = W * H;
        ty = a.type + (int64_t)e * HW;
        co = a.colour + (int64_t)e * HW;
        st = a.state ? a.state + (int64_t)e * HW : nullptr;
        vm = a.vis_mask ? a.vis_mask + (int64_t)e * V * V : nullptr;
        const int dir = a.agent_dir[(int64_t)e * a.astride] & 3;
        mg_view_top(a.agent_x[(int64_t)e * a.astride], a.agent_y[(int64_t)e * a.astride], dir, V, topx, topy);
        rot = (dir + 1) & 3;
        const uint8_t *c = a.carrying ? a.carrying + (int64_t)e * 3 : nullptr;
        carried = (c && c[0] != 0) ? mg_cell{c[0], c[1], c[2], 3, 0} : mg_cell{1, 0, 0, 3, 0};
    }
    __device__ mg_cell at(int cell) const
    {
        const int j = cell / V, i = cell - j * V;           /* once per cell and workgroup, not per byte */
        const int lit = vm ? vm[i * V + j] != 0 : 1;
        mg_cell q = {2, 5, 0, -1, 0};                       /* Grid.slice: outside the world -> Wall() */
        if (i == V / 2 && j == V - 1) {
            q = carried;
        } else if (!lit) {
            q.type = 1; q.colour = 0;
        } else {
            int si, sj;
            mg_view_to_slice(rot, V, i, j, si, sj);
            const int x = topx + si, y = topy + sj;
            if (x >= 0 && x < W && y >= 0 && y < H) {
                const int o = y * W + x;
                q.type = ty[o]; q.colour = co[o]; q.state = st ? st[o] : 0;
            }
        }
        q.highlight = lit;
        return q;
    }
};

/* Workgroup b of frame o owns the chunks [b * MG_RENDER_CHUNKS, (b + 1) * MG_RENDER_CHUNKS) of the frame, a row of
 * row_store.h (aligned 16-byte stores inside the frame, its two ends byte by byte).  It first resolves the cells of the
 * tile rows its span touches into atlas tile indices (LDS), then every lane builds whole chunks: a chunk walks the
 * frame's bytes as (tile row j, pixel row r, tile column i, byte k of the tile's run of tile_size * 3 bytes), fetching
 * four source bytes at a time while they stay inside one run.  W x H are the frame's cells; what they show is Cells'. */
template <class Cells>
__global__ __launch_bounds__(MG_RENDER_THREADS) void mg_render_kernel(
    typename Cells::args src_args, int N, int W, int H, const int32_t *__restrict__ env_index,
    const uint8_t *__restrict__ atlas, int ts, uint8_t *__restrict__ frame, int64_t pitch, int32_t *__restrict__ error,
    int blocks_per_frame)
{
    extern __shared__ uint16_t tidx[];
    __shared__ int wave_bad[MG_RENDER_THREADS / 64];
    const int tid = threadIdx.x;
    if (tid < MG_RENDER_THREADS / 64) wave_bad[tid] = 0;
    __syncthreads();
    const int o = blockIdx.x / blocks_per_frame, b = blockIdx.x - o * blocks_per_frame;
    const int e = env_index ? env_index[o] : o;
    if (e < 0 || e >= N) {
        if (error && b == 0 && tid == 0) error[o] = 2;
        return;
    }
    const int run = ts * 3, rowB = W * run, B = rowB * ts, tileB = ts * run, HW = W * H;
    const int F = B * H;
    uint8_t *fb = frame + (int64_t)o * pitch;
    const mg_row_span_t<int> g = mg_row_span(mg_row_misalign(fb, 16), F, b, MG_RENDER_CHUNKS, 16);
    const int j0 = g.p_lo / B, j1 = (g.p_hi - 1) / B;       /* tile rows of this workgroup's frame bytes */
    const Cells src(src_args, e, W, H);

    for (int t = tid; t < (j1 - j0 + 1) * W; t += MG_RENDER_THREADS) {
        const mg_cell q = src.at(j0 * W + t);
        int idx = mg_tile_index(q.type, q.colour, q.state, q.agent, q.highlight);
        if (idx < 0) idx = mg_tile_index(1, 0, 0, q.agent, q.highlight);
        tidx[t] = (uint16_t)idx;
    }
    if (b == 0 && error) {                                  /* uniform per workgroup: one workgroup scans the frame's cells */
        int bad = 0;
        for (int cell = tid; cell < HW; cell += MG_RENDER_THREADS) {
            const mg_cell q = src.at(cell);
            bad |= mg_tile_index(q.type, q.colour, 0, -1, 0) < 0;
        }
        if (__ballot(bad) != 0 && (tid & 63) == 0) wave_bad[tid >> 6] = 1;
    }
    __syncthreads();
    if (b == 0 && error && tid == 0) error[o] = (wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) ? 1 : 0;

    for (int c = g.c0 + tid; c < g.c1; c += MG_RENDER_THREADS)
        mg_row_store(fb, F, c, [&](int p) {
            int j = p / B, rem = p - j * B;
            int r = rem / rowB, xb = rem - r * rowB;
            int i = xb / run, k = xb - i * run;
            j -= j0;
            uint32_t w[4];
#pragma unroll
            for (int d = 0; d < 4; d++) {
                if (k + 4 <= run) {
                    const uint8_t *src_b = atlas + (int)tidx[j * W + i] * tileB + r * run + k;
                    __builtin_memcpy(&w[d], src_b, 4);
                    k += 4;
                    if (k == run) { k = 0; if (++i == W) { i = 0; if (++r == ts) { r = 0; j++; } } }
                } else {
                    uint32_t v = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        v |= (uint32_t)atlas[(int)tidx[j * W + i] * tileB + r * run + k] << (8 * q);
                        if (++k == run) { k = 0; if (++i == W) { i = 0; if (++r == ts) { r = 0; j++; } } }
                    }
                    w[d] = v;
                }
            }
            return make_uint4(w[0], w[1], w[2], w[3]);
        }, [&](int q) {
            const int j = q / B, rem = q - j * B;
            const int r = rem / rowB, xb = rem - r * rowB;
            const int i = xb / run, k = xb - i * run;
            return atlas[(int)tidx[(j - j0) * W + i] * tileB + r * run + k];
        });
}

/* ------------------------------------------------------------------------------------------------ highlight */
/* get_full_render highlights the world cells of the agent's view window (view_map.h): each world cell looks its view
 * cell (vi, vj) up, no scatter. */
__global__ void mg_highlight_mask_kernel(const uint8_t *__restrict__ vis, int N, int W, int H,
                                         const int32_t *__restrict__ agent_x, const int32_t *__restrict__ agent_y,
                                         const int32_t *__restrict__ agent_dir, int astride, int V, uint8_t *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)N * W * H) return;
    const int e = (int)(g / (W * H)), cell = (int)(g - (int64_t)e * W * H);
    const int d = agent_dir[(int64_t)e * astride] & 3;
    int topx, topy, vi, vj;
    mg_view_top(agent_x[(int64_t)e * astride], agent_y[(int64_t)e * astride], d, V, topx, topy);
    const int x = cell % W, y = cell / W;
    mg_view_from_slice((d + 1) & 3, V, x - topx, y - topy, vi, vj);
    uint8_t v = 0;
    if (vi >= 0 && vi < V && vj >= 0 && vj < V) v = vis ? (vis[((int64_t)e * V + vi) * V + vj] != 0) : 1;
    out[g] = v;
}

/* ------------------------------------------------------------------------------------------------ C ABI */
static void mg_fill_consts(mg_render_consts *k)
{
    for (int d = 0; d < 4; d++) {
        volatile double theta = 0.5 * M_PI * d;             /* volatile: libm at run time, as math.cos / math.sin */
        k->cs[d] = cos(-theta);
        k->sn[d] = sin(-theta);
    }
    volatile float ax = 0.12f, ay = 0.19f, bx = 0.87f, by = 0.50f, cx = 0.12f, cy = 0.81f;
    const float v0x = cx - ax, v0y = cy - ay, v1x = bx - ax, v1y = by - ay;
    const float dot00 = v0x * v0x + v0y * v0y, dot01 = v0x * v1x + v0y * v1y, dot11 = v1x * v1x + v1y * v1y;
    const float inv_denom = 1 / (dot00 * dot11 - dot01 * dot01);
    k->ax = ax; k->ay = ay; k->v0x = v0x; k->v0y = v0y; k->v1x = v1x; k->v1y = v1y;
    k->dot00 = dot00; k->dot01 = dot01; k->dot11 = dot11; k->inv_denom = inv_denom;
}

extern "C" int mg_render_tile_index(int type, int colour, int state, int agent_dir, int highlight)
{
    return mg_tile_index(type, colour, state, agent_dir, highlight);
}

extern "C" int64_t mg_render_atlas_bytes(int tile_size)
{
    if (tile_size < 1 || tile_size > MG_RENDER_MAX_TILE) return TW_E_ARG;
    return (int64_t)MG_RENDER_TILES * tile_size * tile_size * 3;
}

extern "C" int mg_render_constants(double *out18)
{
    if (!out18) return TW_E_ARG;
    mg_render_consts k;
    mg_fill_consts(&k);
    static_assert(sizeof(k) == MG_RENDER_NCONST * sizeof(double), "mg_render_consts is 18 doubles");
    memcpy(out18, &k, sizeof(k));
    return TW_OK;
}

extern "C" int mg_render_build_atlas(int tile_size, uint8_t *atlas, void *stream)
{
    if (!atlas || tile_size < 1 || tile_size > MG_RENDER_MAX_TILE) return TW_E_ARG;
    mg_render_consts k;
    mg_fill_consts(&k);
    hipLaunchKernelGGL(mg_render_atlas_kernel, dim3(MG_RENDER_TILES), dim3(MG_RENDER_THREADS), 0, (hipStream_t)stream,
                       tile_size, atlas, k);
    return tw_launched(__func__);
}

/* The frame-side argument rules and launch geometry of both entry points: n_out frames of width x height cells. */
template <class Cells>
static int mg_launch_frames(const typename Cells::args &src, int n_envs, int width, int height, const int32_t *env_index,
                            int n_out, const uint8_t *atlas, int tile_size, uint8_t *frame, int64_t frame_pitch,
                            int32_t *error, void *stream)
{
    if (!atlas || !frame || n_envs <= 0 || width <= 0 || height <= 0 || n_out <= 0) return TW_E_ARG;
    if (tile_size < 1 || tile_size > MG_RENDER_MAX_TILE) return TW_E_ARG;
    if (!env_index && n_out > n_envs) return TW_E_ARG;
    const int64_t band = (int64_t)width * tile_size * tile_size * 3, fbytes = band * height;
    if (fbytes >= ((int64_t)1 << 31) - 64 || (int64_t)width * height >= ((int64_t)1 << 31)) return TW_E_ARG;
    if (frame_pitch != 0 && frame_pitch < fbytes) return TW_E_ARG;
    const int64_t pitch = frame_pitch ? frame_pitch : fbytes;
    const int64_t bpf = (mg_row_chunks(fbytes, 16) + MG_RENDER_CHUNKS - 1) / MG_RENDER_CHUNKS;
    if (bpf * n_out >= ((int64_t)1 << 31)) return TW_E_ARG;
    int64_t bands = ((int64_t)MG_RENDER_CHUNKS * 16 + band - 1) / band + 1;      /* tile rows one workgroup can touch */
    if (bands > height) bands = height;
    const int64_t lds = bands * width * (int64_t)sizeof(uint16_t);
    if (lds > 48 * 1024) return TW_E_ARG;
    hipLaunchKernelGGL(mg_render_kernel<Cells>, dim3((unsigned)(bpf * n_out)), dim3(MG_RENDER_THREADS), (size_t)lds,
                       (hipStream_t)stream, src, n_envs, width, height, env_index, atlas, tile_size, frame, pitch, error,
                       (int)bpf);
    return tw_launched(__func__);
}

extern "C" int mg_render(const uint8_t *type, const uint8_t *colour, const uint8_t *state, int n_envs, int width,
                         int height, const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_dir,
                         int agent_stride, const int32_t *env_index, int n_out, const uint8_t *highlight,
                         const uint8_t *atlas, int tile_size, uint8_t *frame, int64_t frame_pitch, int32_t *error,
                         void *stream)
{
    if (!type || !colour || !agent_x || !agent_y || !agent_dir || agent_stride <= 0) return TW_E_ARG;
    const mg_world_cells::args src = {type, colour, state, highlight, agent_x, agent_y, agent_dir, agent_stride};
    return mg_launch_frames<mg_world_cells>(src, n_envs, width, height, env_index, n_out, atlas, tile_size, frame,
                                            frame_pitch, error, stream);
}

extern "C" int mg_render_pov(const uint8_t *type, const uint8_t *colour, const uint8_t *state, int n_envs, int width,
                             int height, const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_dir,
                             int agent_stride, const uint8_t *carrying, const int32_t *env_index, int n_out,
                             const uint8_t *vis_mask, int view_size, const uint8_t *atlas, int tile_size, uint8_t *frame,
                             int64_t frame_pitch, int32_t *error, void *stream)
{
    if (!type || !colour || !agent_x || !agent_y || !agent_dir || agent_stride <= 0) return TW_E_ARG;
    if (width <= 0 || height <= 0 || (int64_t)width * height >= ((int64_t)1 << 31)) return TW_E_ARG;
    if (view_size < 1 || view_size > MG_MAX_VIEW) return TW_E_ARG;
    const mg_view_cells::args src = {type, colour, state, carrying, vis_mask, agent_x, agent_y, agent_dir, agent_stride,
                                     width, height};
    return mg_launch_frames<mg_view_cells>(src, n_envs, view_size, view_size, env_index, n_out, atlas, tile_size, frame,
                                           frame_pitch, error, stream);
}

extern "C" int mg_highlight_mask(const uint8_t *vis_mask, int n_envs, int width, int height, const int32_t *agent_x,
                                 const int32_t *agent_y, const int32_t *agent_dir, int agent_stride, int view_size,
                                 uint8_t *out, void *stream)
{
    if (!agent_x || !agent_y || !agent_dir || !out) return TW_E_ARG;
    if (n_envs <= 0 || width <= 0 || height <= 0 || agent_stride <= 0) return TW_E_ARG;
    if (view_size < 1 || view_size > MG_MAX_VIEW || (int64_t)width * height >= ((int64_t)1 << 31)) return TW_E_ARG;
    const int64_t cells = (int64_t)n_envs * width * height;
    if ((cells + 255) / 256 >= ((int64_t)1 << 31)) return TW_E_ARG;
    hipLaunchKernelGGL(mg_highlight_mask_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       vis_mask, n_envs, width, height, agent_x, agent_y, agent_dir, agent_stride, view_size, out);
    return tw_launched(__func__);
}
