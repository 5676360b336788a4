// emu_deflate_dynamic.cpp -- TEST INFRASTRUCTURE.  Builds the Deflate encoder's dynamic-block path (csrc/deflate_comp.h,
// SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC) and the shared Huffman builder (csrc/huffman_wave.h) for the HOST (g++
// -DSWC_HOST_EMULATION), as emu.cpp does for the other kernels: the threads of every SIMT region (csrc/simt.h) one after
// another in a selectable order.  Never shipped, never linked into libswc_hip.so.
#include <cstring>
#include "../../swcompression_amd/csrc/deflate_comp.h"
#include "../../swcompression_amd/csrc/huffman_wave.h"

extern "C" void emu_set_order(int o) { swc::simt::g_order = o; }

// Deflate compression with dynamic blocks: job.in = the buffer, job.aux bit 0 = a segment of a longer stream
extern "C" void emu_deflate_compress_dynamic(swc::Job* jobs, size_t n) {
    alignas(16) static swc::defc::DynLds lds;
    for (size_t g = 0; g < n; g++) {
        std::memset(&lds, 0xEE, sizeof lds);
        swc::defc::deflate_compress_dynamic_job<64>(jobs[g], &lds);
    }
}

// the shared builder on its own: weights w[0 .. alpha) (alpha <= 288) -> code lengths and canonical codes (MSB first)
extern "C" void emu_huffman(const uint32_t* w, uint32_t alpha, uint32_t max_len, uint32_t* len, uint32_t* code) {
    alignas(16) static swc::huff::HuffLds<swc::defc::kHuffCap> l;
    std::memset(&l, 0xEE, sizeof l);
    for (uint32_t s = 0; s < alpha; s++) l.w[s] = w[s];
    swc::huff::huffman_wave<64>(&l, alpha, max_len);
    for (uint32_t s = 0; s < alpha; s++) { len[s] = l.len[s]; code[s] = l.wt[s] & 0xFFFFFFu; }
}
