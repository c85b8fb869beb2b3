// tune_caller.cpp — the kernel files' launch options and their resolvers (uc-tcp-ip_amd/csrc/netcsum_tune.h)
// as a plain C++ program: tests/test_tune_cpu.py builds it with -fsanitize=address,undefined -Wall -Wextra
// -Werror and runs it as a subprocess.
//
// stdin: one case per line, "<field> <value>" — a default-constructed KernelTune with that one field
// set — or "default 0", the struct untouched. stdout: one line per case, the thirteen fields and then
// every resolver, those with a kernel's default as argument once per default the launchers pass.
#include <stdio.h>
#include <string.h>

#include "netcsum_tune.h"

using netcsum::KernelTune;

namespace {

struct Field {
    const char* name;
    int KernelTune::*at;
};
const Field kFields[] = {
    {"stream_waves", &KernelTune::stream_waves}, {"stream_touch", &KernelTune::stream_touch},
    {"stream_xcd", &KernelTune::stream_xcd},     {"tx_flush", &KernelTune::tx_flush},
    {"crc_kernel", &KernelTune::crc_kernel},     {"crc_nt", &KernelTune::crc_nt},
    {"crc_lanes", &KernelTune::crc_lanes},       {"crc_wide", &KernelTune::crc_wide},
    {"hdr_burst", &KernelTune::hdr_burst},       {"varlen_run_bytes", &KernelTune::varlen_run_bytes},
    {"live_compact", &KernelTune::live_compact}, {"store_gather", &KernelTune::store_gather},
    {"chain_grid", &KernelTune::chain_grid},
};

}  // namespace

int main() {
    static_assert(sizeof(KernelTune) == sizeof(kFields) / sizeof(kFields[0]) * sizeof(int), "thirteen ints, all listed");
    char name[64];
    int value = 0;
    while (scanf("%63s %d", name, &value) == 2) {
        KernelTune k;
        if (strcmp(name, "default") != 0) {
            const Field* f = nullptr;
            for (const Field& c : kFields) {
                if (strcmp(c.name, name) == 0) f = &c;
            }
            if (f == nullptr) {
                fprintf(stderr, "no field %s\n", name);
                return 2;
            }
            k.*(f->at) = value;
        }
        for (const Field& c : kFields) printf("%s=%d ", c.name, k.*(c.at));
        for (int w = 0; w <= 9; ++w) printf("lds_bytes(%d)=%u ", w, netcsum::stream_lds_bytes(k, w));
        printf("waves_tuned=%d ", (int)netcsum::stream_waves_tuned(k));
        for (int on = 0; on <= 1; ++on) {
            printf("touch(%d)=%d xcd(%d)=%d ", on, (int)netcsum::stream_touch(k, on != 0), on, (int)netcsum::stream_xcd(k, on != 0));
        }
        const unsigned modes[] = {0u, 1u, 256u};
        for (unsigned m : modes) printf("xcd_mode(%u)=%u ", m, netcsum::stream_xcd_mode(k, m));
        printf("live_compact()=%d store_gather()=%d run_bytes()=%u hdr_burst()=%d chain_grid()=%d tx_flush_mode()=%d\n",
               (int)netcsum::live_compact(k), (int)netcsum::store_gather(k), netcsum::varlen_run_bytes(k),
               (int)netcsum::hdr_burst(k), netcsum::chain_grid(k), netcsum::tx_flush_mode(k));
    }
    return 0;
}
