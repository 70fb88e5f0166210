// TEST ONLY (CPU): the host side of passiveradar_amd/csrc/order_select.h -- the order-preserving keys, their inverses and
// NumPy's percentile rank -- behind C entry points, so tests/test_order_select_host.py can hold them to NumPy without a GPU.
#include "../../passiveradar_amd/csrc/order_select.h"

extern "C" {

void osh_okey_f32(const float* x, uint32_t* k, int n) { for (int i = 0; i < n; ++i) k[i] = prc_okey(x[i]); }
void osh_okey_raw_f32(const float* x, uint32_t* k, int n) { for (int i = 0; i < n; ++i) k[i] = prc_okey_raw(x[i]); }
void osh_key_value_f32(const uint32_t* k, float* x, int n) { for (int i = 0; i < n; ++i) x[i] = prc_key_value(k[i]); }

void osh_okey_f64(const double* x, unsigned long long* k, int n) { for (int i = 0; i < n; ++i) k[i] = prc_okey(x[i]); }
void osh_okey_raw_f64(const double* x, unsigned long long* k, int n) { for (int i = 0; i < n; ++i) k[i] = prc_okey_raw(x[i]); }
void osh_key_value_f64(const unsigned long long* k, double* x, int n) { for (int i = 0; i < n; ++i) x[i] = prc_key_value(k[i]); }

void osh_percentile_rank(double p, uint32_t n, uint32_t* k, double* t) { prc_percentile_rank(p, n, k, t); }

}
