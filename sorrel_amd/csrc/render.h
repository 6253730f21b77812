#pragma once
// render.h -- sprite frames of the world tensor: gather a tile per cell, paste the layers bottom-up, stream the RGBA out.
//
//   render_kernel<TW, VEC, LDS_ATLAS>
//       One WORK ITEM is `rpi` consecutive tile rows of one frame: rpi * th pixel rows of cols * tw pixels, which are CONTIGUOUS bytes
//       of `out` (per plane).  The host makes an item as large as the LDS cell table allows while the launch still has two items per
//       resident workgroup: what an item costs before its first store -- a chain of dependent loads (cell bytes, agents) behind
//       everybody's stores, and three barriers -- is paid once per item (a 32 x 32 map: once per frame, 1 MiB).  Resident
//       workgroups walk the items (block b takes b, b + gridDim, ...), so the atlas, type_tile and the tile flags are brought into
//       LDS once per workgroup and neighbouring workgroups write neighbouring spans.  Per item: the tile of every cell of its rows
//       (type_tile[cell byte], the out-of-map tile, then the agents' tiles) goes to LDS together with the tile's flags and, per
//       cell column, the lowest layer that can still be seen; then lane = one unit of VEC pixels (VEC = 4: 16 bytes), consecutive
//       lanes walk the span, and the first lane of every wave sits on a 128-byte line of `out` (the span is entered `head` units
//       early and the units in front of it are skipped).  Stores are non-temporal: a frame is never read back by this kernel.
//       TW is the tile width when it is a power of two the build has an instance for (16, 8, 32), 0 = any width.
//
// The paste is PIL's masked paste on RGBA, all four bytes alike:  t = dst * (255 - a) + src * a + 128;  out = ((t >> 8) + t) >> 8
// with a = the source pixel's alpha.  Two bytes of a pixel are blended at once in the 16-bit halves of a 32-bit register (t never
// exceeds 255 * 255 + 128, and (t >> 8) + t stays under 65536).  Integer arithmetic only.

constexpr int kRenderMaxCells = 4096;     // layers * cols of one tile row (LDS tables below)
constexpr int kRenderMaxCols = 1024;
constexpr int kRenderAtlasPad = 64;       // bytes between two tiles in LDS: tiles of 1 KiB would otherwise share all their banks
constexpr int kRenderAtlasLds = 44 * 1024;
constexpr int kRenderFlagLds = 2048;      // tile flags kept in LDS up to this many tiles (read through the cache beyond)
constexpr int kRenderStaticLds = 19 * 1024;   // the tables below, rounded up
constexpr int kTileOpaque = 1, kTileClear = 2;

struct RenderParams {
    const uint8_t* grid;
    const uint8_t* atlas;
    const uint8_t* tile_flags;
    const uint16_t* type_tile;
    const uint8_t* agent_pos;
    const uint16_t* agent_tile;
    const int64_t* env_ids;
    const int16_t* centres;
    uint8_t* out;
    int64_t E, n, env_stride, items, span_bytes;
    int L, H, W, A, agent_layer, n_tiles, th, tw, k, vision, oob_tile, per_layer;
    int rows, cols;             // tiles of one frame
    int rpi, items_per_frame;   // tile rows of one work item; items of one frame
    int units_per_row;          // cols * tw / VEC
    int tile_bytes, tile_pitch; // th * tw * 4; the same + the LDS padding
};

__device__ __forceinline__ uint32_t blend_px(uint32_t dst, uint32_t src) {
    const uint32_t a = src >> 24, na = 255u - a;
    uint32_t lo = (dst & 0x00FF00FFu) * na + (src & 0x00FF00FFu) * a + 0x00800080u;
    uint32_t hi = ((dst >> 8) & 0x00FF00FFu) * na + ((src >> 8) & 0x00FF00FFu) * a + 0x00800080u;
    lo = ((((lo >> 8) & 0x00FF00FFu) + lo) >> 8) & 0x00FF00FFu;
    hi = ((((hi >> 8) & 0x00FF00FFu) + hi) >> 8) & 0x00FF00FFu;
    return lo | (hi << 8);
}

template <int VEC>
struct RenderPx {
    uint32_t v[VEC];
};

template <int VEC, bool LDS_ATLAS>
__device__ __forceinline__ RenderPx<VEC> render_fetch(const RenderParams& p, const uint8_t* s_atlas, int tile, int in_tile_px) {
    RenderPx<VEC> r;
    if constexpr (VEC == 4) {
        typedef uint32_t vu4 __attribute__((ext_vector_type(4)));
        vu4 q;
        if constexpr (LDS_ATLAS) q = *reinterpret_cast<const vu4*>(s_atlas + tile * p.tile_pitch + in_tile_px * 4);
        else q = *reinterpret_cast<const vu4*>(p.atlas + (int64_t)tile * p.tile_bytes + in_tile_px * 4);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        if constexpr (LDS_ATLAS) r.v[0] = *reinterpret_cast<const uint32_t*>(s_atlas + tile * p.tile_pitch + in_tile_px * 4);
        else r.v[0] = *reinterpret_cast<const uint32_t*>(p.atlas + (int64_t)tile * p.tile_bytes + in_tile_px * 4);
    }
    return r;
}

template <int VEC>
__device__ __forceinline__ void render_store(uint8_t* at, const RenderPx<VEC>& r) {
    if constexpr (VEC == 4) {
        typedef uint32_t vu4 __attribute__((ext_vector_type(4)));
        vu4 q = {r.v[0], r.v[1], r.v[2], r.v[3]};
        __builtin_nontemporal_store(q, reinterpret_cast<vu4*>(at));
    } else {
        __builtin_nontemporal_store(r.v[0], reinterpret_cast<uint32_t*>(at));
    }
}

template <int TW, int VEC, bool LDS_ATLAS>
__global__ __launch_bounds__(kBlock) void render_kernel(const RenderParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_atlas[];
    __shared__ uint16_t s_tile[kRenderMaxCells];
    __shared__ uint8_t s_flag[kRenderMaxCells];
    __shared__ uint8_t s_base[kRenderMaxCells];
    __shared__ uint16_t s_tt[256];
    __shared__ uint8_t s_tf[kRenderFlagLds];
    const int tid = threadIdx.x;
    const int tw = TW ? TW : p.tw;
    constexpr int kUnit = VEC * 4;                      // bytes a lane stores
    constexpr int kLine = 128 / kUnit;                  // units of one 128-byte line

    if constexpr (LDS_ATLAS) {
        // (tile_bytes is a multiple of 16 on this path: the host takes it only when the atlas is 16-byte aligned and tw % 4 == 0 ... or
        // copies 4 bytes at a time)
        const int per_tile = p.tile_bytes / kUnit;
        for (int i = tid; i < p.n_tiles * per_tile; i += kBlock) {
            const int t = i / per_tile, o = (i - t * per_tile) * kUnit;
            if constexpr (VEC == 4) {
                typedef uint32_t vu4 __attribute__((ext_vector_type(4)));
                *reinterpret_cast<vu4*>(s_atlas + t * p.tile_pitch + o) = *reinterpret_cast<const vu4*>(p.atlas + (int64_t)t * p.tile_bytes + o);
            } else {
                *reinterpret_cast<uint32_t*>(s_atlas + t * p.tile_pitch + o) = *reinterpret_cast<const uint32_t*>(p.atlas + (int64_t)t * p.tile_bytes + o);
            }
        }
    }

    for (int i = tid; i < 256; i += kBlock) s_tt[i] = p.type_tile[i];
    const bool lds_flags = p.tile_flags && p.n_tiles <= kRenderFlagLds;
    if (lds_flags)
        for (int i = tid; i < p.n_tiles; i += kBlock) s_tf[i] = p.tile_flags[i];

    const int planes = p.per_layer ? p.L : 1;
    const int dpy = kBlock / p.units_per_row, dq = kBlock - dpy * p.units_per_row;
    for (int64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const int64_t frame = item / p.items_per_frame;
        const int r0 = (int)(item - frame * p.items_per_frame) * p.rpi;
        const int nr = min(p.rpi, p.rows - r0);
        const int64_t sel = frame / p.k;
        const int64_t env = p.env_ids ? p.env_ids[sel] : sel;
        if (env < 0 || env >= p.E) continue;            // (uniform over the workgroup: no barrier is skipped by part of it)
        int y0 = r0, x0 = 0;
        if (p.centres) {
            y0 = (int)p.centres[frame * 2] - p.vision + r0;
            x0 = (int)p.centres[frame * 2 + 1] - p.vision;
        }
        const uint8_t* g = p.grid + env * p.env_stride;
        const int row_cells = p.L * p.cols;
        __syncthreads();                                // the previous item's readers are done with the tables (and the atlas is in)
        for (int i = tid; i < nr * row_cells; i += kBlock) {
            const int rr = i / row_cells, j = i - rr * row_cells;
            const int l = j / p.cols, c = j - l * p.cols, x = x0 + c, y = y0 + rr;
            int t = p.oob_tile;
            if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
                t = s_tt[g[((int64_t)l * p.H + y) * p.W + x]];
                if (t >= p.n_tiles) t = p.oob_tile;
            }
            s_tile[i] = (uint16_t)t;
        }
        __syncthreads();
        if (p.agent_pos) {
            for (int a = tid; a < p.A; a += kBlock) {
                const int ay = p.agent_pos[(env * p.A + a) * 2], ax = p.agent_pos[(env * p.A + a) * 2 + 1];
                const int t = p.agent_tile[env * p.A + a];
                const int c = ax - x0, rr = ay - y0;
                if (rr >= 0 && rr < nr && ay < p.H && ax < p.W && c >= 0 && c < p.cols && t < p.n_tiles)
                    s_tile[(rr * p.L + p.agent_layer) * p.cols + c] = (uint16_t)t;
            }
        }
        __syncthreads();
        for (int i = tid; i < nr * p.cols; i += kBlock) {
            const int rr = i / p.cols, c = i - rr * p.cols;
            int base = 0;
            for (int l = 0; l < p.L; ++l) {
                const int at = (rr * p.L + l) * p.cols + c;
                const uint8_t f = lds_flags ? s_tf[s_tile[at]] : (p.tile_flags ? p.tile_flags[s_tile[at]] : (uint8_t)0);
                s_flag[at] = f;
                if (f & kTileOpaque) base = l;
            }
            s_base[i] = (uint8_t)base;
        }
        __syncthreads();

        const int64_t span_units = (int64_t)nr * p.span_bytes / kUnit;
        for (int plane = 0; plane < planes; ++plane) {
            uint8_t* span = p.out + ((frame * planes + plane) * p.rows + r0) * p.span_bytes;
            const int head = (int)((reinterpret_cast<uintptr_t>(span) / kUnit) & (kLine - 1));
            int64_t u = tid - head;
            if (u < 0) u += kBlock;
            if (u >= span_units) continue;
            const int py0 = (int)(u / p.units_per_row);
            int q = (int)(u - (int64_t)py0 * p.units_per_row);
            int rr = py0 / p.th, iy = py0 - rr * p.th;                  // tile row of the item, pixel row of the tile
            for (; u < span_units; u += kBlock) {
                const int px = q * VEC;
                int c, ix;
                if constexpr (TW == 16) { c = px >> 4; ix = px & 15; }
                else if constexpr (TW == 8) { c = px >> 3; ix = px & 7; }
                else if constexpr (TW == 32) { c = px >> 5; ix = px & 31; }
                else { c = px / tw; ix = px - c * tw; }
                const int in_tile = iy * tw + ix;
                const int cell = rr * row_cells + c;
                RenderPx<VEC> acc;
                if (p.per_layer) {
                    acc = render_fetch<VEC, LDS_ATLAS>(p, s_atlas, s_tile[cell + plane * p.cols], in_tile);
                } else {
                    int l = s_base[rr * p.cols + c];
                    acc = render_fetch<VEC, LDS_ATLAS>(p, s_atlas, s_tile[cell + l * p.cols], in_tile);
                    for (++l; l < p.L; ++l) {
                        if (s_flag[cell + l * p.cols] & kTileClear) continue;
                        const RenderPx<VEC> src = render_fetch<VEC, LDS_ATLAS>(p, s_atlas, s_tile[cell + l * p.cols], in_tile);
#pragma unroll
                        for (int j = 0; j < VEC; ++j) acc.v[j] = blend_px(acc.v[j], src.v[j]);
                    }
                }
                render_store<VEC>(span + u * kUnit, acc);
                iy += dpy;
                q += dq;
                if (q >= p.units_per_row) { q -= p.units_per_row; ++iy; }
                while (iy >= p.th) { iy -= p.th; ++rr; }
            }
        }
    }
}

// host side: the instance for a tile width
template <int VEC, bool LDS>
void launch_render(const RenderParams& p, unsigned blocks, size_t lds, hipStream_t s) {
    switch (p.tw) {
    case 16: hipLaunchKernelGGL((render_kernel<16, VEC, LDS>), dim3(blocks), dim3(kBlock), lds, s, p); break;
    case 8: hipLaunchKernelGGL((render_kernel<8, VEC, LDS>), dim3(blocks), dim3(kBlock), lds, s, p); break;
    case 32: hipLaunchKernelGGL((render_kernel<32, VEC, LDS>), dim3(blocks), dim3(kBlock), lds, s, p); break;
    default: hipLaunchKernelGGL((render_kernel<0, VEC, LDS>), dim3(blocks), dim3(kBlock), lds, s, p); break;
    }
}
