// cda_wave.hpp - the wave toolkit of the readers (cda_tape*.inc, cda_book_report.inc, cda_quotes.inc, cda_stylised.inc, cda_tape_pnl.inc) and of the scripted
// book walks (cda_scripted.inc, cda_scripted_label.inc): what a one-wave-per-market reduction needs besides its own arithmetic.  cda_hip.hip includes it ahead of
// every .inc; everything here is __forceinline__ and leaves no symbol behind.  A new reader starts here, with the record accessors beside TapeSpan (cda_tape.inc)
// and QuoteSpan (cda_quotes.inc) and with reader_launch (cda_hip.hip).
#pragma once

// ---- who am I: wave `w` of the launch (one wave per market, or per side of a market) and the lane; workgroups are whole waves.  A kernel that keeps a slice of
// LDS per wave also needs `wib`, its wave's place in the workgroup, and names the workgroup's waves: CDA_WPB, or (int)(blockDim.x >> 6) where the host sizes
// the workgroup by the LDS a wave takes.  Both give the same w; they are two because each compiles to what the kernels had before they shared it.
#define READER_WAVE() const int w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63)
#define READER_WAVE_IN_GROUP(waves) const int wib = (int)(threadIdx.x >> 6), w = (int)blockIdx.x * (waves) + wib, lane = (int)(threadIdx.x & 63)

// ---- reductions over the 64 lanes: every lane ends with the result
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ long long wave_min(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ long long wave_max(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// ---- inclusive scans over the lanes: lane l ends with the sum / the maximum over lanes 0 .. l
__device__ __forceinline__ long long wave_scan_sum(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { const long long o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}
__device__ __forceinline__ long long wave_scan_max(long long x, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { const long long y = __shfl_up(x, d); if (lane >= d && y > x) x = y; }
    return x;
}
__device__ __forceinline__ int wave_scan_max(int x, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d && y > x) x = y; }
    return x;
}
// lanes 0 .. lane of a 64-bit lane mask
__device__ __forceinline__ unsigned long long lanes_le(int lane) { return ~0ull >> (63 - lane); }

// ---- a signed value added to an unsigned 64-bit word of the wave's own slice of LDS (two's complement: the sum reads back as a long long; the order cannot matter)
__device__ __forceinline__ void lds_add(unsigned long long* p, long long v) { atomicAdd(p, (unsigned long long)v); }

// ---- the four-word info row of wave w (callers: one lane, and only where the caller asked for the rows).  A macro: as an inlined function it changed the code
// of k_tape_pnl and k_quote_stats around the store.
#define reader_info(info, w, a, b, c, d) do { int32_t* o_ = (info) + 4 * (size_t)(w); o_[0] = (a); o_[1] = (b); o_[2] = (c); o_[3] = (d); } while (0)
