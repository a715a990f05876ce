// Writes the stream twiddle table the library uploads (yagi_amd/csrc/stream_tables.hpp, the builder capi.hip calls) to
// stdout as raw float32 pairs, and behind it as uint32 the slot of every entry of the scaled correction table (512) and
// of the scaled FFT{h} (4096), the two device tables the filter object lays out in the same pairs;
// tests/test_stream_tables_cpu.py builds and reads it.
#include <cstdio>
#include <vector>

#include "stream_tables.hpp"

struct cf { float re, im; };

int main() {
    std::vector<cf> tab(yagi::kStreamTabFloat2);
    yagi::build_stream_twiddles(tab.data());
    if (std::fwrite(tab.data(), sizeof(cf), tab.size(), stdout) != tab.size()) return 1;
    std::vector<unsigned> slot(512);
    for (unsigned k = 0; k < 512; ++k) slot[k] = yagi::stream_gc_slot(k);
    if (std::fwrite(slot.data(), sizeof(unsigned), slot.size(), stdout) != slot.size()) return 1;
    slot.resize(4096);
    for (unsigned k = 0; k < 4096; ++k) slot[k] = yagi::stream_hs_slot(k);
    if (std::fwrite(slot.data(), sizeof(unsigned), slot.size(), stdout) != slot.size()) return 1;
    return 0;
}
