// crc32.hip — CRC-32 (zlib / IEEE 802.3: reflected polynomial 0xEDB88320, init and final xor
// 0xFFFFFFFF) of every block of a batch, parallel inside a block.
//
// CRC is linear over GF(2). raw(M) = the register after feeding M from state 0, no final xor;
// Z_k(s) = the register s after k zero bytes = s * x^(8k) mod P. Then
//   raw(A | B) = Z_|B|(raw(A)) ^ raw(B),   crc32(M) = ~(Z_|M|(0xFFFFFFFF) ^ raw(M)),
// and leading zero bytes leave raw unchanged. With T_k[v] = Z_k(T_0[v]) (the slice-by-N tables),
// a byte v followed by k more bytes contributes T_k[v], and Z_k(s) for k >= 4 is
// T_{k-1}[s0] ^ T_{k-2}[s1] ^ T_{k-3}[s2] ^ T_{k-4}[s3] over the four bytes of s.
//
// crc32_tiles: every block is cut into block-relative tiles of kCrcTile bytes (no tile straddles
//   two blocks); one wave takes a tile as its aligned 16-byte chunks, chunk c on lane c % 64
//   (coalesced 1 KiB rows). A lane runs Horner over its chunks, which lie kCrcRow bytes apart:
//   s = Z_1024(s) ^ raw(chunk) = 4 + 16 table lookups in LDS per 16 bytes. A lane's value then
//   moves to the end of the last chunk by one multiplication with x^(128 j), j = chunks that
//   follow its last one (< 64), and the wave XOR-reduces. The tile's start may be any byte: the
//   first chunk is loaded whole and the bytes before the start zeroed; the bytes after the last
//   whole chunk (< 16) are fed one at a time by lane 0.
// crc32_fold: one wave per block. Lane l runs Horner over a contiguous run of the block's full
//   tiles (s = s * x^(8 kCrcTile) ^ partial, as many steps as the block has tiles per lane: a
//   block of 2^32 - 2 bytes has 4096), moves its value to the block's end (a product over the
//   set bits of the byte count, from the x^(8 2^k) table), the wave XOR-reduces, and lane 0 adds
//   the short last tile and Z_n(0xFFFFFFFF).
// No atomics, no scratch: the result is deterministic.
#include "device_util.h"

#include <mutex>

namespace bmh {

constexpr uint32_t kCrcTile = 16384;  // bytes a wave takes at a time (16 rows)
constexpr uint32_t kCrcRow = 1024;    // 64 lanes x 16 bytes
constexpr uint32_t kCrcTabs = 20;     // T_0..T_15 (chunk bytes), T_1020..T_1023 (Horner step)
// constants buffer (u32 words): the tables, x^(128 j) for j < 64, x^(8 2^k) for k < 40
constexpr uint32_t kCrcLaneK = kCrcTabs * 256, kCrcXp = kCrcLaneK + 64, kCrcConsts = kCrcXp + 40;
// LDS of crc32_tiles: the tables and the lane constants; 7 workgroups (28 waves) fit a CU
constexpr uint32_t kCrcLdsBudget = 21 * 1024;
static_assert((kCrcLaneK + 64) * 4 <= kCrcLdsBudget && 7 * kCrcLdsBudget <= 160 * 1024,
              "crc32_tiles: LDS for 7 workgroups a CU");
static_assert(kCrcTile % kCrcRow == 0 && kCrcTile == 1u << 14, "crc32_fold steps by x^(8 2^14)");

struct CrcBlk {
    uint32_t off, n, tile0;  // byte offset in the batch, length, index of the first tile
};

// s after the 16 bytes of v, which lie 1024 bytes after the chunk s ended with
__device__ __forceinline__ uint32_t crc_step(const uint32_t *tab, uint32_t s, uint4 v)
{
    auto t = [&](uint32_t k, uint32_t w, uint32_t sh) { return tab[k * 256 + ((w >> sh) & 0xffu)]; };
    const uint32_t a = t(19, s, 0) ^ t(18, s, 8) ^ t(17, s, 16) ^ t(16, s, 24);
    const uint32_t b = t(15, v.x, 0) ^ t(14, v.x, 8) ^ t(13, v.x, 16) ^ t(12, v.x, 24);
    const uint32_t c = t(11, v.y, 0) ^ t(10, v.y, 8) ^ t(9, v.y, 16) ^ t(8, v.y, 24);
    const uint32_t d = t(7, v.z, 0) ^ t(6, v.z, 8) ^ t(5, v.z, 16) ^ t(4, v.z, 24);
    const uint32_t e = t(3, v.w, 0) ^ t(2, v.w, 8) ^ t(1, v.w, 16) ^ t(0, v.w, 24);
    return (a ^ b) ^ (c ^ d) ^ e;
}

// dword d of a chunk whose first `head` bytes (1..15) lie before the tile: those bytes zeroed
__device__ __forceinline__ uint32_t crc_head_mask(uint32_t w, uint32_t d, uint32_t head)
{
    if (head >= 4 * d + 4) return 0;
    if (head <= 4 * d) return w;
    return w & (0xffffffffu << (8 * (head - 4 * d)));
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x ^= __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(256) void crc32_tiles(const uint8_t *__restrict__ in, const CrcBlk *__restrict__ blk,
                                                   uint32_t nb, uint32_t ntiles, const uint32_t *__restrict__ cst,
                                                   uint32_t *__restrict__ part)
{
    __shared__ uint32_t tab[kCrcLaneK + 64];
    for (uint32_t i = threadIdx.x; i < kCrcLaneK + 64; i += 256) tab[i] = cst[i];
    __syncthreads();
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t t = blockIdx.x * 4 + w; t < ntiles; t += gridDim.x * 4) {
        uint32_t lo = 0, hi = nb - 1;  // the block of tile t: the last one with tile0 <= t
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (blk[mid].tile0 <= t) lo = mid;
            else hi = mid - 1;
        }
        const CrcBlk B = blk[lo];
        const uint32_t rel = (t - B.tile0) * kCrcTile, len = min(kCrcTile, B.n - rel);
        const uint8_t *p = in + ((uint64_t)B.off + rel);  // the tile: [p, p + len)
        const uint32_t head = (uint32_t)((uintptr_t)p & 15u);  // bytes of the first chunk before the tile
        const uint8_t *pa = p - head;                     // 16-byte aligned
        const uint32_t C = (head + len) >> 4;             // whole chunks from pa: <= 1024
        uint32_t s = 0;
        // four rows at a time: the loads first (a lane past the end re-reads the last chunk and
        // drops it), so they are in flight together
        for (uint32_t c0 = 0; c0 < C; c0 += 256) {
            uint4 v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                v[k] = *(const uint4 *)(pa + 16 * (size_t)min(c0 + 64 * k + l, C - 1));
            if (c0 == 0 && l == 0 && head) {
                v[0].x = crc_head_mask(v[0].x, 0, head);
                v[0].y = crc_head_mask(v[0].y, 1, head);
                v[0].z = crc_head_mask(v[0].z, 2, head);
                v[0].w = crc_head_mask(v[0].w, 3, head);
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t s2 = crc_step(tab, s, v[k]);
                s = c0 + 64 * k + l < C ? s2 : s;
            }
        }
        // lane l's last chunk is followed by (C - 1 - l) % 64 chunks
        s = l < C ? crc32_mul(s, tab[kCrcLaneK + ((C - 1 - l) & 63u)]) : 0u;
        s = wave_xor(s);
        if (l == 0) {
            for (uint32_t i = C ? 16 * C - head : 0; i < len; ++i) s = tab[(s ^ p[i]) & 0xffu] ^ (s >> 8);
            part[t] = s;
        }
    }
}

// x^(8 nbytes) mod P from the x^(8 2^k) table
__device__ __forceinline__ uint32_t crc_xpow8(const uint32_t *__restrict__ xp, uint32_t nbytes)
{
    uint32_t r = 0x80000000u;
    for (uint32_t k = 0; nbytes; ++k, nbytes >>= 1)
        if (nbytes & 1u) r = crc32_mul(r, xp[k]);
    return r;
}

__global__ __launch_bounds__(64) void crc32_fold(const CrcBlk *__restrict__ blk, const uint32_t *__restrict__ part,
                                                 const uint32_t *__restrict__ cst, uint32_t *__restrict__ crc)
{
    const CrcBlk B = blk[blockIdx.x];
    const uint32_t l = threadIdx.x, *xp = cst + kCrcXp;
    const uint32_t full = (uint32_t)(((uint64_t)B.n + kCrcTile - 1) / kCrcTile) - 1;  // all tiles but the last
    const uint32_t per = (full + 63) / 64, t0 = min(full, l * per), t1 = min(full, t0 + per);
    const uint32_t xt = xp[14];
    uint32_t s = 0;
    for (uint32_t t = t0; t < t1; ++t) s = crc32_mul(s, xt) ^ part[B.tile0 + t];
    s = t1 > t0 ? crc32_mul(s, crc_xpow8(xp, B.n - t1 * kCrcTile)) : 0u;
    s = wave_xor(s);
    if (l == 0) crc[blockIdx.x] = ~(crc32_mul(0xffffffffu, crc_xpow8(xp, B.n)) ^ s ^ part[B.tile0 + full]);
}

static const uint32_t *crc_consts_host()
{
    static std::vector<uint32_t> v;
    static std::once_flag once;
    std::call_once(once, [] {
        v.resize(kCrcConsts);
        std::vector<uint32_t> t(crc32_table0(), crc32_table0() + 256);
        auto z1 = [&](uint32_t s) { return crc32_table0()[s & 0xffu] ^ (s >> 8); };
        for (uint32_t k = 0; k < 1024; ++k) {  // t = T_k
            if (k < 16 || k >= 1020) memcpy(&v[(k < 16 ? k : k - 1020 + 16) * 256], t.data(), 1024);
            for (auto &x : t) x = z1(x);
        }
        for (uint32_t j = 0; j < 64; ++j) v[kCrcLaneK + j] = crc32_xpow8(16 * j);
        for (uint32_t k = 0; k < 40; ++k) v[kCrcXp + k] = crc32_xpow8(1ull << k);
    });
    return v.data();
}

void crc32_batch(Ctx *c, const uint8_t *d_in, const Batch &bt, uint32_t *d_crc)
{
    uint32_t *d_cst = (uint32_t *)c->get(WS_CRC_TAB, kCrcConsts * 4);
    if (!c->ws_tag[WS_CRC_TAB]) {
        c->h2d(d_cst, crc_consts_host(), kCrcConsts * 4);
        c->ws_tag[WS_CRC_TAB] = 1;
    }
    std::vector<CrcBlk> hb(bt.nblocks);
    uint32_t ntiles = 0;
    for (uint32_t b = 0; b < bt.nblocks; ++b) {
        const uint64_t n = bt.offs[b + 1] - bt.offs[b];
        hb[b] = CrcBlk{(uint32_t)bt.offs[b], (uint32_t)n, ntiles};
        ntiles += cdiv(n, kCrcTile);
    }
    CrcBlk *d_blk = (CrcBlk *)c->get(WS_CRC_BLK, hb.size() * sizeof(CrcBlk));
    uint32_t *d_part = (uint32_t *)c->get(WS_CRC_PART, (size_t)ntiles * 4);
    c->h2d(d_blk, hb.data(), hb.size() * sizeof(CrcBlk));
    const uint32_t grid = std::min<uint32_t>(cdiv(ntiles, 4), (uint32_t)c->cus * 7);
    BMH_LAUNCH(c, "crc32_tiles", crc32_tiles, grid, 256, 0, d_in, d_blk, bt.nblocks, ntiles, d_cst, d_part);
    BMH_LAUNCH(c, "crc32_fold", crc32_fold, bt.nblocks, 64, 0, d_blk, d_part, d_cst, d_crc);
}

}  // namespace bmh
