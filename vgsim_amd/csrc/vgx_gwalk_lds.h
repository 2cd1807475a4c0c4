// vgx_gwalk_lds.h — the log reader of the device walks (vgx_genealogies.hip, vgx_lineages.hip): records of the device event log
// are prefetched VGX_GW_CHUNK at a time into a column of the workgroup's LDS buffer, one round trip to HBM per chunk instead of
// one per event.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VGX_GW_CHUNK 8   // log records per prefetch (8 x 24 bytes per lane; 12 KB of LDS per 64-lane workgroup)

// reads log records from an LDS copy of the chunk that holds them; records [e0, e0 + CHUNK) are loaded as 8-byte words
struct VgxGwLdsReader {
    const int32_t *log;   // the replicate's slot 0
    int64_t n;            // records in the log
    int32_t *lds;         // this lane's column of the workgroup's buffer
    int64_t chunk;
    __device__ void load(int64_t ch) {
        chunk = ch;
        const int64_t e0 = ch * VGX_GW_CHUNK;
        const int m = (int)(n - e0 < VGX_GW_CHUNK ? n - e0 : VGX_GW_CHUNK);
        const int2 *src = (const int2 *)(log + e0 * 6);   // 8-byte aligned: records are 24 bytes from a 256-byte aligned base
        int2 v[3 * VGX_GW_CHUNK];
#pragma unroll
        for (int j = 0; j < 3 * VGX_GW_CHUNK; j++) v[j] = j < 3 * m ? src[j] : make_int2(0, 0);
#pragma unroll
        for (int j = 0; j < 3 * VGX_GW_CHUNK; j++) { lds[(2 * j) * 64] = v[j].x; lds[(2 * j + 1) * 64] = v[j].y; }
    }
    __device__ void at(int64_t e, int32_t c[5]) {
        const int64_t ch = e / VGX_GW_CHUNK;
        if (ch != chunk) load(ch);
        const int j = (int)(e - ch * VGX_GW_CHUNK) * 6;
#pragma unroll
        for (int i = 0; i < 5; i++) c[i] = lds[(j + i) * 64];
    }
};
