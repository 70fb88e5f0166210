// TEST ONLY, host only: hands out the two twiddle tables exactly as libprcore builds them (fftw_make_tables of caf_fft.hip,
// ft_make_tables of caf_fft_team.hip -- the library's own functions, reached by linking against it), for the table test
// that runs without a GPU.  No kernel, no HIP call.
#include "../../passiveradar_amd/csrc/fft_team.h"

// wave: FFTW_TABLE float2 (1152), team: FT_GTAB float2 (4352); either may be null.  Returns the two lengths packed as
// FFTW_TABLE | FT_GTAB << 16 so that the caller can size its buffers from the library's own constants.
extern "C" int fft_probe_tables(void* wave, void* team) {
    if (wave) fftw_make_tables(static_cast<float2*>(wave));
    if (team) ft_make_tables(static_cast<float2*>(team));
    return FFTW_TABLE | (FT_GTAB << 16);
}
