// xeve_amd/csrc/md5_core.h -- the decoded-picture signature (xeve_md5_imgb, src_base/xeve_util.c:1067-1083; xeve_md5_init / _update / _finish, :895-1065): a standard
// MD5 (RFC 1321) of a plane's interior -- h rows of w 16-bit little-endian samples, rows following one another without padding -- as what ONE lane of md5.hip runs.
// __host__ __device__ and plain C++: tests/native/md5_host.cpp compiles the same source for the host and holds it to hashlib without a GPU.
//   transform     the 64 steps over one 64-byte block; the four state words and the sixteen message words are named registers (every index is a constant)
//   Reader / take the message in order: 32 samples per block, gathered across row boundaries (rows are `stride` samples apart in memory, `w` samples long)
//   finish        the last, partial block with both padding branches (the 0x80 byte and the 64-bit bit count fit the block up to 55 message bytes; from 56 on a second
//                 block carries the count)
// MD5 is one serial chain per message: the parallel axis is the messages (md5.hip: a lane each).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define XM __host__ __device__ inline __attribute__((always_inline))
#else
#define XM inline __attribute__((always_inline))
#endif

namespace xmd5 {

struct State {
    uint32_t a, b, c, d;
};
XM void init(State &s) { s.a = 0x67452301u, s.b = 0xefcdab89u, s.c = 0x98badcfeu, s.d = 0x10325476u; }
XM uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); } // (one v_alignbit_b32 on the device)

#define XM_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define XM_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define XM_H(x, y, z) ((x) ^ (y) ^ (z))
#define XM_I(x, y, z) ((y) ^ ((x) | ~(z)))
#define XM_STEP(f, a, b, c, d, k, t, r) a = b + rotl(a + f(b, c, d) + m[k] + t, r)
XM void transform(State &s, const uint32_t m[16])
{
    uint32_t a = s.a, b = s.b, c = s.c, d = s.d;
    XM_STEP(XM_F, a, b, c, d, 0, 0xd76aa478u, 7), XM_STEP(XM_F, d, a, b, c, 1, 0xe8c7b756u, 12), XM_STEP(XM_F, c, d, a, b, 2, 0x242070dbu, 17), XM_STEP(XM_F, b, c, d, a, 3, 0xc1bdceeeu, 22);
    XM_STEP(XM_F, a, b, c, d, 4, 0xf57c0fafu, 7), XM_STEP(XM_F, d, a, b, c, 5, 0x4787c62au, 12), XM_STEP(XM_F, c, d, a, b, 6, 0xa8304613u, 17), XM_STEP(XM_F, b, c, d, a, 7, 0xfd469501u, 22);
    XM_STEP(XM_F, a, b, c, d, 8, 0x698098d8u, 7), XM_STEP(XM_F, d, a, b, c, 9, 0x8b44f7afu, 12), XM_STEP(XM_F, c, d, a, b, 10, 0xffff5bb1u, 17), XM_STEP(XM_F, b, c, d, a, 11, 0x895cd7beu, 22);
    XM_STEP(XM_F, a, b, c, d, 12, 0x6b901122u, 7), XM_STEP(XM_F, d, a, b, c, 13, 0xfd987193u, 12), XM_STEP(XM_F, c, d, a, b, 14, 0xa679438eu, 17), XM_STEP(XM_F, b, c, d, a, 15, 0x49b40821u, 22);
    XM_STEP(XM_G, a, b, c, d, 1, 0xf61e2562u, 5), XM_STEP(XM_G, d, a, b, c, 6, 0xc040b340u, 9), XM_STEP(XM_G, c, d, a, b, 11, 0x265e5a51u, 14), XM_STEP(XM_G, b, c, d, a, 0, 0xe9b6c7aau, 20);
    XM_STEP(XM_G, a, b, c, d, 5, 0xd62f105du, 5), XM_STEP(XM_G, d, a, b, c, 10, 0x02441453u, 9), XM_STEP(XM_G, c, d, a, b, 15, 0xd8a1e681u, 14), XM_STEP(XM_G, b, c, d, a, 4, 0xe7d3fbc8u, 20);
    XM_STEP(XM_G, a, b, c, d, 9, 0x21e1cde6u, 5), XM_STEP(XM_G, d, a, b, c, 14, 0xc33707d6u, 9), XM_STEP(XM_G, c, d, a, b, 3, 0xf4d50d87u, 14), XM_STEP(XM_G, b, c, d, a, 8, 0x455a14edu, 20);
    XM_STEP(XM_G, a, b, c, d, 13, 0xa9e3e905u, 5), XM_STEP(XM_G, d, a, b, c, 2, 0xfcefa3f8u, 9), XM_STEP(XM_G, c, d, a, b, 7, 0x676f02d9u, 14), XM_STEP(XM_G, b, c, d, a, 12, 0x8d2a4c8au, 20);
    XM_STEP(XM_H, a, b, c, d, 5, 0xfffa3942u, 4), XM_STEP(XM_H, d, a, b, c, 8, 0x8771f681u, 11), XM_STEP(XM_H, c, d, a, b, 11, 0x6d9d6122u, 16), XM_STEP(XM_H, b, c, d, a, 14, 0xfde5380cu, 23);
    XM_STEP(XM_H, a, b, c, d, 1, 0xa4beea44u, 4), XM_STEP(XM_H, d, a, b, c, 4, 0x4bdecfa9u, 11), XM_STEP(XM_H, c, d, a, b, 7, 0xf6bb4b60u, 16), XM_STEP(XM_H, b, c, d, a, 10, 0xbebfbc70u, 23);
    XM_STEP(XM_H, a, b, c, d, 13, 0x289b7ec6u, 4), XM_STEP(XM_H, d, a, b, c, 0, 0xeaa127fau, 11), XM_STEP(XM_H, c, d, a, b, 3, 0xd4ef3085u, 16), XM_STEP(XM_H, b, c, d, a, 6, 0x04881d05u, 23);
    XM_STEP(XM_H, a, b, c, d, 9, 0xd9d4d039u, 4), XM_STEP(XM_H, d, a, b, c, 12, 0xe6db99e5u, 11), XM_STEP(XM_H, c, d, a, b, 15, 0x1fa27cf8u, 16), XM_STEP(XM_H, b, c, d, a, 2, 0xc4ac5665u, 23);
    XM_STEP(XM_I, a, b, c, d, 0, 0xf4292244u, 6), XM_STEP(XM_I, d, a, b, c, 7, 0x432aff97u, 10), XM_STEP(XM_I, c, d, a, b, 14, 0xab9423a7u, 15), XM_STEP(XM_I, b, c, d, a, 5, 0xfc93a039u, 21);
    XM_STEP(XM_I, a, b, c, d, 12, 0x655b59c3u, 6), XM_STEP(XM_I, d, a, b, c, 3, 0x8f0ccc92u, 10), XM_STEP(XM_I, c, d, a, b, 10, 0xffeff47du, 15), XM_STEP(XM_I, b, c, d, a, 1, 0x85845dd1u, 21);
    XM_STEP(XM_I, a, b, c, d, 8, 0x6fa87e4fu, 6), XM_STEP(XM_I, d, a, b, c, 15, 0xfe2ce6e0u, 10), XM_STEP(XM_I, c, d, a, b, 6, 0xa3014314u, 15), XM_STEP(XM_I, b, c, d, a, 13, 0x4e0811a1u, 21);
    XM_STEP(XM_I, a, b, c, d, 4, 0xf7537e82u, 6), XM_STEP(XM_I, d, a, b, c, 11, 0xbd3af235u, 10), XM_STEP(XM_I, c, d, a, b, 2, 0x2ad7d2bbu, 15), XM_STEP(XM_I, b, c, d, a, 9, 0xeb86d391u, 21);
    s.a += a, s.b += b, s.c += c, s.d += d;
}
#undef XM_STEP
#undef XM_F
#undef XM_G
#undef XM_H
#undef XM_I

// where the message stands: `row` = the first sample of the row being read, `col` = the next sample's column.  Only samples [0, w) of rows [0, h) are ever read.
struct Reader {
    const uint16_t *row;
    int64_t         stride; // samples from one row to the next
    int32_t         w, col;
};
XM uint32_t next(Reader &r) // one sample, as it lies in memory
{
    const uint32_t v = r.row[r.col];
    if(++r.col == r.w) r.col = 0, r.row += r.stride;
    return v;
}
struct Quad {
    uint32_t v[4];
};
// the next 64 bytes of the message as sixteen little-endian words.  A block that lies inside one row is read in 16-byte or 4-byte pieces where its address allows
// (the picture stores' rows start on 16-byte boundaries and are a whole number of blocks long at the common sizes); otherwise sample by sample across the row's end
XM void take(Reader &r, uint32_t m[16])
{
    const uint16_t *p = r.row + r.col;
    const uintptr_t at = (uintptr_t)p;
    if(r.col + 32 <= r.w && (at & 3) == 0) {
        if((at & 15) == 0) {
            for(int q = 0; q < 4; q++) {
                Quad t;
                __builtin_memcpy(&t, __builtin_assume_aligned(p + 8 * q, 16), 16);
                m[4 * q] = t.v[0], m[4 * q + 1] = t.v[1], m[4 * q + 2] = t.v[2], m[4 * q + 3] = t.v[3];
            }
        }
        else
            for(int k = 0; k < 16; k++) __builtin_memcpy(&m[k], __builtin_assume_aligned(p + 2 * k, 4), 4);
        if((r.col += 32) == r.w) r.col = 0, r.row += r.stride;
        return;
    }
    for(int k = 0; k < 16; k++) {
        const uint32_t lo = next(r);
        m[k] = lo | (next(r) << 16);
    }
}
// the message's last `rem` samples (0 .. 31), the padding and the length; bytes = the WHOLE message's length (64 bits: a plane of 8192 x 4320 samples is 2^26 bytes, but
// the leaf takes any h x w)
XM void finish(State &s, Reader &r, int rem, uint64_t bytes)
{
    uint32_t m[16];
    for(int k = 0; k < 16; k++) {
        const uint32_t lo = 2 * k < rem ? next(r) : 2 * k == rem ? 0x80u : 0u;
        const uint32_t hi = 2 * k + 1 < rem ? next(r) : 2 * k + 1 == rem ? 0x80u : 0u;
        m[k] = lo | (hi << 16);
    }
    if(rem >= 28) { // 56 message bytes or more: the count does not fit behind the 0x80 byte
        transform(s, m);
        for(int k = 0; k < 14; k++) m[k] = 0;
    }
    const uint64_t bits = bytes << 3;
    m[14] = (uint32_t)bits, m[15] = (uint32_t)(bits >> 32);
    transform(s, m);
}
// the digest of h rows of w samples at p, rows `stride` samples apart (w, h >= 1): what hashlib.md5 gives for the rows' bytes joined
XM void digest_plane(const uint16_t *p, int64_t stride, int32_t w, int32_t h, uint8_t out[16])
{
    State s;
    init(s);
    Reader r = {p, stride, w, 0};
    const uint64_t samples = (uint64_t)w * (uint64_t)h, blocks = samples >> 5;
    if(blocks) {
        // the next block's loads are issued ahead of the current block's 64 dependent steps
        uint32_t cur[16], nxt[16];
        take(r, cur);
        for(uint64_t b = 1; b < blocks; b++) {
            take(r, nxt);
            transform(s, cur);
            for(int k = 0; k < 16; k++) cur[k] = nxt[k];
        }
        transform(s, cur);
    }
    finish(s, r, (int)(samples & 31), samples * 2);
    const uint32_t v[4] = {s.a, s.b, s.c, s.d};
    for(int k = 0; k < 16; k++) out[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
}

} // namespace xmd5
