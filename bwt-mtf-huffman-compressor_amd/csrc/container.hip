// container.hip — the BMH container as a device-resident object: written, decoded,
// verified and read by byte ranges with the stream and the plain bytes both in HBM. Only
// O(nblocks) metadata crosses PCIe: the 32-byte header, the record-length and CRC tables, the
// first bytes of each record (its 24-byte header) and status words.
//
//   compress_d2d   : batches of at most BMH_OPT_MAX_BATCH bytes through encode_blocks into the
//                    context's output workspace, one device-to-device copy per batch to the
//                    records' (byte-aligned) place, the tables built on the host and copied up last.
//   decompress_d2d : the tables and record headers come down, decode_blocks decodes the records
//                    where they lie straight into the caller's buffer; CRCs by crc32_batch.
//   readv_d2d      : the blocks some range touches are decoded once into the workspace, and
//                    k_gather_pieces copies every (range, block) intersection to its place in the
//                    output in one launch.
#include "bmh_internal.h"

#include <algorithm>

namespace bmh {

namespace {

// Long pieces are cut into tiles on the host, one workgroup each (the kernel itself is correct
// for any length: the cut only spreads a long piece over the device).
constexpr uint64_t kGatherTile = 64u << 10;
constexpr uint32_t kHead = 32;  // bytes of each record brought to the host (record_n reads 25)

// One workgroup per piece: byte head up to the destination's 16-byte boundary, a body of
// 16-byte stores, byte tail. The body loads 16 bytes where the source is co-aligned, four dwords
// where it is dword-aligned, and otherwise the five aligned dwords that hold its 16 bytes,
// shifted into place: every load is an aligned word that holds at least one byte of the piece's
// source, and no store touches a byte outside the piece's destination.
__global__ __launch_bounds__(256) void k_gather_pieces(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                       const Piece *__restrict__ pieces)
{
    const Piece p = pieces[blockIdx.x];
    const uint8_t *s = src + p.src;
    uint8_t *d = dst + p.dst;
    const uint32_t t = threadIdx.x;
    const uint64_t to16 = (0 - (uintptr_t)d) & 15u, head = p.len < to16 ? p.len : to16;
    if (t < head) d[t] = s[t];
    const uint8_t *sb = s + head;
    uint4 *db = (uint4 *)(d + head);
    const uint64_t nvec = (p.len - head) >> 4;
    const uint32_t sh = (uint32_t)((uintptr_t)sb & 3u);
    if (((uintptr_t)sb & 15u) == 0) {
        const uint4 *q = (const uint4 *)sb;
        for (uint64_t i = t; i < nvec; i += 256) db[i] = q[i];
    } else if (sh == 0) {
        const uint32_t *q = (const uint32_t *)sb;
        for (uint64_t i = t; i < nvec; i += 256) db[i] = make_uint4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    } else {
        const uint32_t *q = (const uint32_t *)(sb - sh);
        const uint32_t lo = 8 * sh, hi = 32 - lo;
        for (uint64_t i = t; i < nvec; i += 256) {
            const uint32_t *w = q + 4 * i;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            db[i] = make_uint4((w0 >> lo) | (w1 << hi), (w1 >> lo) | (w2 << hi), (w2 >> lo) | (w3 << hi),
                               (w3 >> lo) | (w4 << hi));
        }
    }
    const uint64_t done = head + 16 * nvec;
    if (t < p.len - done) d[done + t] = s[done + t];
}

// d2h + sync of a few bytes into memory that goes with the caller's frame
void fetch(Ctx *c, void *h_dst, const void *d_src, size_t bytes)
{
    if (!bytes) return;
    try {
        c->d2h(h_dst, d_src, bytes);
        c->sync();
    } catch (...) {
        c->deferred.clear();  // no later sync may write h_dst
        throw;
    }
}

// The stream's record list, as parse_container gives it for a host buffer: the header and then
// the tables come down, nothing else. A bare record is one block (version 0; block_size and total
// are left 0 for the caller, who reads the record's header).
ContainerView stream_view(Ctx *c, const uint8_t *d_in, uint64_t len)
{
    uint8_t head[32] = {0};
    const uint64_t hl = std::min<uint64_t>(len, 32);
    fetch(c, head, d_in, hl);
    const int version = container_version(head, hl);
    if (!version) {
        ContainerView v;
        v.version = 0;
        v.block_size = v.total = 0;
        v.nblocks = 1;
        v.rec_off.push_back(0);
        v.rec_len.push_back(len);
        return v;
    }
    if (len < 32) fail(BMH_ECORRUPT, "container: bad magic");  // (as parse_container: shorter than its header)
    const uint64_t nb = get_u64(head + 16);
    if (nb == 0 || nb > (len - 32) / (version == 2 ? 12 : 8)) fail(BMH_ECORRUPT, "container: bad block count");
    // parse_container reads the tables only, and checks that they fit `len` before it does
    std::vector<uint8_t> tab(std::min(len, container_table_bytes(version, nb)));
    memcpy(tab.data(), head, 32);
    fetch(c, tab.data() + 32, d_in + 32, tab.size() - 32);
    return parse_container(tab.data(), len);
}

// The first kHead bytes (or all, if fewer) of records blocks[0..] of the view, kHead bytes apart
// and zero-filled, gathered on the device and brought down in one copy.
std::vector<uint8_t> record_heads(Ctx *c, const uint8_t *d_in, const ContainerView &v, const std::vector<uint64_t> &blocks)
{
    std::vector<uint8_t> heads(blocks.size() * kHead, 0);
    std::vector<Piece> pieces;
    pieces.reserve(blocks.size());
    for (size_t i = 0; i < blocks.size(); ++i)
        pieces.push_back(Piece{v.rec_off[blocks[i]], i * kHead, std::min<uint64_t>(kHead, v.rec_len[blocks[i]])});
    uint8_t *d_heads = (uint8_t *)c->get(WS_HEADS, heads.size());
    BMH_HIP(hipMemsetAsync(d_heads, 0, heads.size(), c->stream));
    gather_pieces(c, d_in, d_heads, pieces);
    fetch(c, heads.data(), d_heads, heads.size());
    return heads;
}

bool overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? na > y - x : nb > x - y;
}

}  // namespace

void gather_pieces(Ctx *c, const uint8_t *d_src, uint8_t *d_dst, const std::vector<Piece> &pieces)
{
    std::vector<Piece> tiles;
    tiles.reserve(pieces.size());
    for (const Piece &p : pieces)
        for (uint64_t o = 0; o < p.len; o += kGatherTile)  // (tiles keep the piece's relative alignment)
            tiles.push_back(Piece{p.src + o, p.dst + o, std::min(kGatherTile, p.len - o)});
    if (tiles.empty()) return;
    if (tiles.size() > 0x7fffffffull) fail(BMH_ERANGE, "gather: too many pieces");
    Piece *d_pieces = (Piece *)c->get(WS_PIECES, tiles.size() * sizeof(Piece));
    c->h2d(d_pieces, tiles.data(), tiles.size() * sizeof(Piece));
    BMH_LAUNCH(c, "gather_pieces", k_gather_pieces, (uint32_t)tiles.size(), 256, 0, d_src, d_dst, d_pieces);
}

void compress_d2d(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t block_size, uint8_t *d_out, uint64_t out_cap,
                  uint64_t *out_len)
{
    if (!d_in || !d_out || !out_len) fail(BMH_EINVAL, "null argument");
    if (n == 0) fail(BMH_EINVAL, "empty input (the reference segfaults on empty input)");
    if ((uintptr_t)d_out & 7u) fail(BMH_EINVAL, "compress: the output must be 8-byte aligned");
    if (overlap(d_in, n, d_out, out_cap)) fail(BMH_EINVAL, "compress: input and output overlap");
    const uint64_t bs = (block_size == 0 || block_size >= n) ? n : block_size;
    if (bs >= 0xffffffffull) fail(BMH_ERANGE, "block size must be < 4 GiB - 1");
    const uint64_t nblocks = (n + bs - 1) / bs;
    const bool checksum = c->opt.checksum != 0;  // BMH_OPT_CHECKSUM: a version-2 container, always
    const uint64_t table = checksum ? container_table_bytes(2, nblocks) : nblocks == 1 ? 0 : 32 + 8 * nblocks;
    if (table > out_cap) fail(BMH_ERANGE, "compress: output capacity too small");
    std::vector<uint8_t> head(table, 0);  // header, record lengths, CRCs and their padding
    std::vector<uint32_t> crcs(checksum ? nblocks : 0);
    const uint64_t cap_batch = max_batch_bytes(c);
    uint64_t at = table;
    std::vector<uint64_t> offs, ro;
    for (uint64_t b0 = 0; b0 < nblocks;) {
        // as encode_host_blocks cuts its batches; make_batch's own limits besides
        offs.assign(1, 0);
        uint64_t cap = 0, b = b0;
        for (; b < nblocks && b - b0 < 65535; ++b) {
            const uint64_t len = std::min(bs, n - b * bs);
            if (b > b0 && (offs.back() + len > cap_batch || offs.back() + len >= 0xffffffffull)) break;
            offs.push_back(offs.back() + len);
            cap += bmh_record_bound(len);
        }
        const uint32_t nb = (uint32_t)(b - b0);
        const Batch bt = make_batch(offs.data(), nb);
        const uint8_t *d_blk = d_in + b0 * bs;
        uint8_t *d_ws = (uint8_t *)c->get(WS_OUT, cap);
        ro.assign(nb + 1, 0);
        if (checksum) {  // of the plain bytes, ahead of the encode on the context's stream
            uint32_t *d_crc = (uint32_t *)c->get(WS_CRC_OUT, (size_t)nb * 4);
            crc32_batch(c, d_blk, bt, d_crc);
            c->d2h(crcs.data() + b0, d_crc, (size_t)nb * 4);
        }
        try {
            encode_blocks(c, d_blk, bt, d_ws, cap, ro.data(), 16);
            if (checksum) c->sync();  // the CRCs have landed (the encode may have run on sub-pipelines)
        } catch (...) {
            c->deferred.clear();  // `crcs` goes with this call: no later sync may write it
            throw;
        }
        const uint64_t bytes = ro[nb];
        if (bytes > out_cap - at) fail(BMH_ERANGE, "compress: output capacity too small");
        // the next batch's pipelines write the workspace from streams of their own: the copy is
        // waited for here
        BMH_HIP(hipMemcpyAsync(d_out + at, d_ws, bytes, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
        for (uint32_t i = 0; table && i < nb; ++i) put_u64(head.data() + 32 + 8 * (b0 + i), ro[i + 1] - ro[i]);
        at += bytes;
        b0 = b;
    }
    if (table) {
        memcpy(head.data(), checksum ? kContainerMagic2 : kContainerMagic, 8);
        put_u64(head.data() + 8, bs);
        put_u64(head.data() + 16, nblocks);
        put_u64(head.data() + 24, n);
        for (uint64_t b = 0; b < crcs.size(); ++b)
            for (int k = 0; k < 4; ++k) head[32 + 8 * nblocks + 4 * b + k] = (uint8_t)(crcs[b] >> (8 * k));
        c->h2d(d_out, head.data(), table);
        c->sync();
    }
    *out_len = at;
}

void decompress_d2d(Ctx *c, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t cap, uint64_t *n_out,
                    bool verify, uint64_t *bad)
{
    // as decompress_dev (capi.cpp), with the record list and the record headers fetched from HBM
    const ContainerView v = stream_view(c, d_in, len);
    const size_t nrec = v.rec_off.size();
    std::vector<uint64_t> all(nrec);
    for (size_t b = 0; b < nrec; ++b) all[b] = b;
    const std::vector<uint8_t> heads = record_heads(c, d_in, v, all);
    uint64_t total = 0;
    std::vector<uint64_t> ns(nrec);
    for (size_t b = 0; b < nrec; ++b) {
        ns[b] = record_n(&heads[b * kHead], v.rec_len[b]);
        total += ns[b];
    }
    *n_out = total;
    if (!verify) {
        if (!d_out) return;
        if (total > cap) fail(BMH_ERANGE, "decompress: output capacity too small");
        if (overlap(d_in, len, d_out, total)) fail(BMH_EINVAL, "decompress: input and output overlap");
    }
    std::vector<uint32_t> got;
    const uint64_t cap_batch = max_batch_bytes(c);
    uint64_t done = 0;
    for (size_t i = 0; i < nrec;) {
        size_t j = i;
        uint64_t nout = 0;
        while (j < nrec && j - i < 65535 && (j == i || nout + ns[j] <= cap_batch)) nout += ns[j++];
        uint8_t *d_o = verify ? (uint8_t *)c->get(WS_OUT, nout + 64) : d_out + done;
        // the records where they lie: absolute offsets (a container's records are back to back)
        std::vector<uint64_t> offs(j - i + 1), oo(j - i + 1, 0);
        for (size_t k = i; k < j; ++k) offs[k - i] = v.rec_off[k];
        offs[j - i] = v.rec_off[j - 1] + v.rec_len[j - 1];
        decode_blocks(c, d_in, offs.data(), (uint32_t)(j - i), d_o, nout, oo.data());
        if (!v.crc.empty()) {  // the CRC-32 of every decoded block, on the device
            got.resize(j - i);
            uint32_t *d_crc = (uint32_t *)c->get(WS_CRC_OUT, (j - i) * 4);
            crc32_batch(c, d_o, make_batch(oo.data(), (uint32_t)(j - i)), d_crc);
            fetch(c, got.data(), d_crc, (j - i) * 4);
            for (size_t k = i; k < j; ++k)
                if (got[k - i] != v.crc[k]) {
                    if (bad) *bad = k;
                    fail_crc(k, v.crc[k], got[k - i]);
                }
        }
        done += nout;
        i = j;
    }
}

void readv_d2d(Ctx *c, const uint8_t *d_in, uint64_t len, const uint64_t *h_offs, const uint64_t *h_counts,
               uint32_t nranges, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_offs, uint64_t *bad)
{
    if (!d_in || !h_out_offs || (nranges && (!h_offs || !h_counts))) fail(BMH_EINVAL, "null argument");
    ContainerView v = stream_view(c, d_in, len);
    std::vector<uint8_t> heads;
    if (v.version == 0) {  // a bare record: one block of its own n bytes
        heads = record_heads(c, d_in, v, {0});
        v.block_size = v.total = record_n(heads.data(), len);
    }
    const uint64_t bs = v.block_size;
    struct Range {
        uint64_t first, count, nread;
    };
    std::vector<Range> rg(nranges);
    uint64_t skip;
    container_locate(bs, v.nblocks, v.total, 0, 0, nullptr, nullptr, nullptr, nullptr);  // the geometry, once
    h_out_offs[0] = 0;
    for (uint32_t r = 0; r < nranges; ++r) {
        container_locate(bs, v.nblocks, v.total, h_offs[r], h_counts[r], &rg[r].first, &rg[r].count, &skip,
                         &rg[r].nread);
        if (rg[r].nread > UINT64_MAX - h_out_offs[r]) fail(BMH_ERANGE, "readv: the ranges total more than 2^64 bytes");
        h_out_offs[r + 1] = h_out_offs[r] + rg[r].nread;
    }
    if (h_out_offs[nranges] > out_cap) fail(BMH_ERANGE, "readv: output capacity too small");
    if (h_out_offs[nranges] == 0) return;
    if (!d_out) fail(BMH_EINVAL, "null argument");
    if (overlap(d_in, len, d_out, h_out_offs[nranges])) fail(BMH_EINVAL, "readv: input and output overlap");

    // the blocks some range touches, in order, and each one's place in that list
    std::vector<int64_t> cover(v.nblocks + 1, 0);
    for (const Range &r : rg)
        if (r.nread) {
            ++cover[r.first];
            --cover[r.first + r.count];
        }
    std::vector<uint64_t> cov, pos(v.nblocks, 0);
    int64_t depth = 0;
    for (uint64_t b = 0; b < v.nblocks; ++b)
        if ((depth += cover[b]) > 0) {
            pos[b] = cov.size();
            cov.push_back(b);
        }
    // every covered record's n against the geometry, before anything is decoded
    if (v.version) heads = record_heads(c, d_in, v, cov);
    std::vector<uint64_t> ns(cov.size());
    for (size_t i = 0; i < cov.size(); ++i) {
        ns[i] = record_n(&heads[i * kHead], v.rec_len[cov[i]]);
        if (ns[i] != std::min(bs, v.total - cov[i] * bs))
            fail(BMH_ECORRUPT, "container: block " + std::to_string(cov[i]) + " holds " + std::to_string(ns[i]) +
                                   " bytes, the header's geometry gives " +
                                   std::to_string(std::min(bs, v.total - cov[i] * bs)));
    }

    const uint64_t cap_batch = max_batch_bytes(c);
    std::vector<uint32_t> got;
    std::vector<Piece> pieces;
    for (size_t i = 0; i < cov.size();) {
        size_t j = i;
        uint64_t nout = 0, nin = 0;
        while (j < cov.size() && j - i < 65535 &&
               (j == i || (nout + ns[j] <= cap_batch && nout + ns[j] < 0xffffffffull))) {
            nout += ns[j];
            nin += v.rec_len[cov[j]];
            ++j;
        }
        const uint32_t nb = (uint32_t)(j - i);
        // consecutive blocks are decoded where they lie; scattered ones are first gathered back to back
        std::vector<uint64_t> offs(nb + 1, 0), oo(nb + 1, 0);
        const uint8_t *d_rec = d_in;
        if (cov[j - 1] - cov[i] == nb - 1) {
            for (size_t k = i; k < j; ++k) offs[k - i] = v.rec_off[cov[k]];
            offs[nb] = v.rec_off[cov[j - 1]] + v.rec_len[cov[j - 1]];
        } else {
            pieces.clear();
            for (size_t k = i; k < j; ++k) {
                pieces.push_back(Piece{v.rec_off[cov[k]], offs[k - i], v.rec_len[cov[k]]});
                offs[k - i + 1] = offs[k - i] + v.rec_len[cov[k]];
            }
            uint8_t *d_recs = (uint8_t *)c->get(WS_IN, nin + 64);
            gather_pieces(c, d_in, d_recs, pieces);
            d_rec = d_recs;
        }
        uint8_t *d_o = (uint8_t *)c->get(WS_OUT, nout + 64);
        decode_blocks(c, d_rec, offs.data(), nb, d_o, nout, oo.data());
        uint32_t *d_crc = nullptr;
        if (!v.crc.empty()) {
            d_crc = (uint32_t *)c->get(WS_CRC_OUT, (size_t)nb * 4);
            crc32_batch(c, d_o, make_batch(oo.data(), nb), d_crc);
        }
        // the (range, block) intersections of this batch: a range's blocks are all covered, so
        // those between the batch's first and last block are in it
        pieces.clear();
        for (uint32_t r = 0; r < nranges; ++r) {
            if (!rg[r].nread || rg[r].first > cov[j - 1] || rg[r].first + rg[r].count <= cov[i]) continue;
            const uint64_t lo = h_offs[r], hi = lo + rg[r].nread;
            for (uint64_t b = std::max(rg[r].first, cov[i]); b <= std::min(rg[r].first + rg[r].count - 1, cov[j - 1]); ++b) {
                const uint64_t s = std::max(lo, b * bs), e = std::min(hi, b * bs + ns[pos[b]]);
                pieces.push_back(Piece{oo[pos[b] - i] + (s - b * bs), h_out_offs[r] + (s - lo), e - s});
            }
        }
        gather_pieces(c, d_o, d_out, pieces);
        if (d_crc) {
            got.resize(nb);
            fetch(c, got.data(), d_crc, (size_t)nb * 4);
            for (size_t k = i; k < j; ++k)
                if (got[k - i] != v.crc[cov[k]]) {
                    if (bad) *bad = cov[k];
                    fail_crc(cov[k], v.crc[cov[k]], got[k - i]);
                }
        } else {
            c->sync();
        }
        i = j;
    }
}

}  // namespace bmh
