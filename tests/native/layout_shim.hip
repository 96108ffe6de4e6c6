// The sizing functions of csrc/wofdm_kernel.h as C symbols, for the CPU test that keeps their Python restatement
// (tests/kernel_cases.py) honest: tests/test_kernel_cases.py.  Host code only; nothing here touches a GPU.
#include "../../w-ofdm-optimization_amd/csrc/wofdm_kernel.h"

extern "C" {
int shim_small_spwr(int n_fft, int S, int B) { return wofdm_small_spwr(n_fft, S, B); }
int shim_waves(int layout, int n_fft, int S, int B) { return wofdm_waves(layout, n_fft, S, B); }
int shim_fbuf_len(int n_fft, int T, int layout, int S, int B) { return wofdm_fbuf_len(n_fft, T, layout, S, B); }
unsigned shim_lds_bytes(int n_fft, int T, int layout, int S, int B) { return wofdm_lds_bytes(n_fft, T, layout, S, B); }
int shim_pick_layout(int n_fft, int S, int B, int plain, int firm, int mdft)
{
    return wofdm_pick_layout(n_fft, S, B, plain != 0, firm != 0, mdft != 0);
}
int shim_pick_layout_masked(int n_fft, int B, int firm) { return wofdm_pick_layout_masked(n_fft, B, firm != 0); }
int shim_layout_built(int layout, int n_fft, int var) { return wofdm_layout_built(layout, n_fft, var) ? 1 : 0; }
}
