// emu_bgzf.cpp -- TEST INFRASTRUCTURE.  The BGZF writer's device code (swcompression_amd/csrc/bgzf_pack.h) and the wave CRC it
// uses, built for the HOST (g++ -DSWC_HOST_EMULATION): the 64 threads of every SIMT region run one after another in the order
// emu_set_order selects.  Part of libswc_emu.so (emu.cpp includes it; tests/_emu_bgzf.py); the writer's CRC launch is
// emu_crc32_wave.  Never shipped.
#include "emu_util.h"
#include "../../swcompression_amd/csrc/bgzf_pack.h"

using swc::Job;
namespace bg = swc::bgzf;

// the workspace plan as the library cuts it: out[0..9) = n, stride, cjobs, kjobs, crcs, offs, res, slots, bytes
extern "C" void emu_bgzf_plan(uint64_t len, uint64_t bs, uint64_t* out) {
    const bg::Plan p = bg::plan(len, bs);
    const uint64_t v[9] = {p.n, p.stride, p.cjobs, p.kjobs, p.crcs, p.offs, p.res, p.slots, p.bytes};
    std::memcpy(out, v, sizeof v);
}

// the set-up kernel: both job lists of `src` cut into chunks of bs bytes, the slots `stride` apart
extern "C" void emu_bgzf_setup(const uint8_t* src, uint64_t len, uint32_t bs, Job* cj, Job* kj, uint8_t* slots, uint64_t stride) {
    const uint64_t n = (len + bs - 1) / bs;
    for (uint64_t g = 0; g * 64 < n; g++) bg::setup_jobs<64>((uint32_t)g, src, len, bs, n, cj, kj, slots, stride);
}

// scan + pack as the two kernels run them.  Member i: its stream of s[i] bytes at slots + i * stride (4-byte aligned, 4 readable
// bytes behind the stream), the status of its compress job, the CRC-32 and the length of its chunk.  Returns Result::status;
// *bad = the member the status is from.
extern "C" int emu_bgzf_pack(const uint8_t* slots, uint64_t stride, const uint32_t* s, const int32_t* status, const uint32_t* crcs,
                             const uint32_t* isizes, uint64_t n, uint8_t* dst, uint64_t dst_cap, int eof, uint64_t* total, uint64_t* sizes,
                             uint64_t* bad) {
    std::vector<Job> cj(n + 1), kj(n + 1);
    std::vector<uint64_t> offs(n + 1, 0xEEEEEEEEEEEEEEEEull);
    for (uint64_t i = 0; i < n; i++) {
        cj[i] = Job{};
        cj[i].out = const_cast<uint8_t*>(slots + i * stride);
        cj[i].out_len = s[i];
        cj[i].status = status[i];
        kj[i] = Job{};
        kj[i].out_len = isizes[i];
    }
    bg::Result res;
    std::memset(&res, 0xEE, sizeof res);
    bg::scan_members<64>(cj.data(), n, offs.data(), sizes, total, &res, dst_cap, eof != 0);
    const uint64_t waves = n + (eof ? 1 : 0);
    for (uint64_t w = 0; w < waves; w++) {   // (the waves of the launch in the order of the regions' threads)
        const uint64_t i = swc::simt::g_order == 1 ? waves - 1 - w : w;
        bg::pack_wave<64>(i, n, cj.data(), kj.data(), crcs, offs.data(), &res, dst, eof != 0);
    }
    if (bad) *bad = res.bad;
    return res.status;
}
