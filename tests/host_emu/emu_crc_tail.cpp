// emu_crc_tail.cpp -- TEST INFRASTRUCTURE.  The CRC tail of the Deflate copy kernel (swcompression_amd/csrc/crc32_tail.h) built
// for the HOST (g++ -DSWC_HOST_EMULATION): the 64 threads of every SIMT region run one after another in the order emu_set_order
// selects.  Part of libswc_emu.so (emu.cpp includes it; tests/_emu_crc_tail.py); never shipped.
#include "emu_util.h"
#include "../../swcompression_amd/csrc/crc32_tail.h"
#include "../../swcompression_amd/csrc/lz_copy.h"

namespace ct = swc::crct;

// the constants of the tail go where the copy kernel's window was, and nowhere else
static_assert(sizeof(ct::TailConsts) <= swc::lzc::CfgDeflate::kWin, "the tail's constants must fit the Deflate window");
static_assert(ct::kTailBytes == 6144, "the window the tail is written for");

// CRC-32 of p[0..n) by the tail, its constants in a buffer of exactly 6,144 bytes between two guards.  Returns 0 and the value
// in *crc, or 1 if a guard byte was touched.
extern "C" int emu_crc_tail(const uint8_t* p, uint32_t n, uint32_t* crc) {
    constexpr size_t kGuard = 64;
    alignas(16) static uint8_t room[kGuard + 6144 + kGuard];
    std::memset(room, 0x5A, sizeof room);
    *crc = ct::crc32_tail(p, n, reinterpret_cast<ct::TailConsts*>(room + kGuard), emu_wave_consts());
    for (size_t i = 0; i < kGuard; i++)
        if (room[i] != 0x5A || room[kGuard + 6144 + i] != 0x5A) return 1;
    return 0;
}
