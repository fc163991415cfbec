/*
 * hap_region.h -- which bytes of a block texture a block-aligned rectangle needs.  Plain C, one definition: the host
 * code (hap_pictures.c, and HapGpuRegionNeedsBytes in hap_api.c) and the kernel that blanks decode units
 * (snappy_decode.hip) include this file and nothing else decides the question.
 *
 * A texture of `width` texels is rows of width / 4 blocks of block_bytes (8 or 16) bytes, row after row.  The region
 * (x, y, w, h in texels, all multiples of 4, w and h non-zero, x + w <= width) holds, of block row r in
 * [y / 4, (y + h) / 4), the bytes [(r * (width / 4) + x / 4) * block_bytes, (r * (width / 4) + (x + w) / 4) * block_bytes).
 */
#ifndef HAP_REGION_H
#define HAP_REGION_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HAP_REGION_FN static inline __host__ __device__
#else
#define HAP_REGION_FN static inline
#endif

/* 1: (x, y, w, h) is a block-aligned, non-empty rectangle of a width-wide texture (the texture's height is the caller's
   to check) */
HAP_REGION_FN int hap_region_geometry_valid(unsigned width, unsigned x, unsigned y, unsigned w, unsigned h)
{
    if (width == 0u || w == 0u || h == 0u || ((width | x | y | w | h) & 3u))
        return 0;
    /* x + w <= width and y + h <= 2^32 - 4 without overflow */
    return x <= width && w <= width - x && h <= 0xFFFFFFFCu - y;
}

/* 1: ... of a texture of block_bytes-byte blocks: the block textures have blocks of 8 or 16 bytes */
HAP_REGION_FN int hap_region_valid(unsigned width, unsigned block_bytes, unsigned x, unsigned y, unsigned w, unsigned h)
{
    return (block_bytes == 8u || block_bytes == 16u) && hap_region_geometry_valid(width, x, y, w, h);
}

/* 1 if and only if bytes [first, first + count) hold at least one byte of a block of the region; 0 for an empty range
   and for arguments hap_region_valid refuses */
HAP_REGION_FN int hap_region_needs_bytes(unsigned width, unsigned block_bytes, unsigned x, unsigned y, unsigned w,
                                         unsigned h, unsigned long long first, unsigned long long count)
{
    unsigned long long stride, lo, hi, last, r;
    if (count == 0u || !hap_region_valid(width, block_bytes, x, y, w, h))
        return 0;
    stride = (unsigned long long)(width / 4u) * block_bytes;            /* bytes of a block row: < 2^34 */
    lo = (unsigned long long)(x / 4u) * block_bytes;                     /* the region's bytes inside a block row: [lo, hi) */
    hi = (unsigned long long)((x + w) / 4u) * block_bytes;
    last = count - 1u > ~0ull - first ? ~0ull : first + (count - 1u);    /* the range's last byte */
    /* the first block row whose region bytes end behind `first`: r * stride + hi > first */
    r = first < hi ? 0u : (first - hi) / stride + 1u;
    if (r < y / 4u)
        r = y / 4u;
    /* (r < 2^30 from here on: r * stride < 2^64) */
    return r < (unsigned long long)(y / 4u) + h / 4u && r * stride + lo <= last;
}

#endif
