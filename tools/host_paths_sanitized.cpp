// The paths of libgss_hip's host code that need no device, under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own (no Python, no GPU; run it on the build
// machine).  From the repository root:
//
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=on -fno-fast-math \
//      -mllvm -amdgpu-mfma-vgpr-form=1 -Xarch_host -fsanitize=address,undefined \
//      -Xarch_host -fno-sanitize-recover=undefined"
//   mkdir -p build/sanitized
//   for u in gss_api stft wpe cacgmm cacgmm_model mvdr chsel posterior_activity wpd; do
//       hipcc $F -c pb_chime5_amd/csrc/$u.hip -o build/sanitized/$u.o || exit 1; done
//   hipcc $F -Iinclude -x hip -c tools/host_paths_sanitized.cpp -o build/sanitized/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/sanitized/*.o \
//       -o build/sanitized/host_paths
//   ASAN_OPTIONS=detect_leaks=0 build/sanitized/host_paths
//
// (detect_leaks=0: the HIP runtime keeps its tables until the process ends.)  It checks the
// geometry helpers against their definitions over the sizes of tests/test_capi_symbols.py, the
// message of a failed gss_create, and that every entry point refuses a NULL context.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "gss_hip.h"

static int failures = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// an entry point with a NULL context and every other argument 0 / NULL
template <typename... A>
static int with_null_context(int (*entry)(gss_ctx *, A...)) {
    return entry(nullptr, A{}...);
}
#define EXPECT_REFUSES_NULL(entry) EXPECT(with_null_context(entry) == GSS_ERR_INVALID)

static void geometry() {
    const int stfts[][2] = {{1024, 256}, {512, 128}, {64, 16}, {4, 2}};
    const int64_t lengths[] = {0, 1, 5, 255, 256, 257, 1000, 1024, 1025, 5000, 16000, 80000, 240000};
    for (const auto &st : stfts) {
        const int size = st[0], shift = st[1];
        for (int fading = 0; fading < 2; ++fading) {
            const int64_t pad = fading ? 2 * (size - shift) : 0;
            for (int64_t n : lengths) {
                const int64_t padded = n + pad;
                const int64_t frames =
                    padded < size ? 1 : (int64_t)std::ceil((double)(padded - size) / shift) + 1;
                EXPECT(gss_stft_num_frames(n, size, shift, fading) == frames);
                EXPECT(gss_samples_to_stft_frames(n, size, shift, fading) ==
                       (int64_t)std::ceil((double)(padded - size + shift) / shift));
                const int64_t samples = frames * shift + size - shift - pad;
                EXPECT(gss_istft_num_samples(frames, size, shift, fading) ==
                       (samples < 0 ? 0 : samples));
            }
        }
    }
}

int main() {
    geometry();
    EXPECT(gss_abi_version() == GSS_ABI_VERSION);
    EXPECT(std::strstr(gss_version(), "gfx950") != nullptr);
    EXPECT(gss_last_error(nullptr) != nullptr);
    EXPECT(gss_create(0, nullptr) == GSS_ERR_INVALID);
    gss_ctx *ctx = nullptr;
    if (gss_create(0, &ctx) == GSS_OK) {    // a device after all: nothing of this needs one
        EXPECT(gss_destroy(ctx) == GSS_OK);
    } else {
        EXPECT(ctx == nullptr);
        EXPECT(std::strlen(gss_last_error(nullptr)) > 0);
    }
    char bus[8];
    EXPECT(gss_device_pci_bus_id(0, bus, (int)sizeof(bus)) == GSS_ERR_INVALID);   // len < 16
    EXPECT(gss_destroy(nullptr) == GSS_OK);
    EXPECT(gss_workspace_bytes(nullptr) == 0);

    EXPECT_REFUSES_NULL(gss_set_stream);
    EXPECT_REFUSES_NULL(gss_set_utterances_in_flight);
    EXPECT_REFUSES_NULL(gss_synchronize);
    EXPECT_REFUSES_NULL(gss_dev_malloc);
    EXPECT_REFUSES_NULL(gss_dev_free);
    EXPECT_REFUSES_NULL(gss_memcpy_h2d);
    EXPECT_REFUSES_NULL(gss_memcpy_d2h);
    EXPECT_REFUSES_NULL(gss_memset);
    EXPECT_REFUSES_NULL(gss_host_malloc);
    EXPECT_REFUSES_NULL(gss_host_free);
    EXPECT_REFUSES_NULL(gss_memcpy_h2d_async);
    EXPECT_REFUSES_NULL(gss_memcpy_d2h_async);
    EXPECT_REFUSES_NULL(gss_profile_enable);
    EXPECT_REFUSES_NULL(gss_profile_filter);
    EXPECT_REFUSES_NULL(gss_profile_reset);
    EXPECT_REFUSES_NULL(gss_profile_report);
    EXPECT_REFUSES_NULL(gss_set_windows);
    EXPECT_REFUSES_NULL(gss_stft);
    EXPECT_REFUSES_NULL(gss_istft);
    EXPECT_REFUSES_NULL(gss_activity_time_to_frequency);
    EXPECT_REFUSES_NULL(gss_wpe);
    EXPECT_REFUSES_NULL(gss_wpe_arrays);
    EXPECT_REFUSES_NULL(gss_wpe_inverse_power);
    EXPECT_REFUSES_NULL(gss_wpe_weighted);
    EXPECT_REFUSES_NULL(gss_cacgmm);
    EXPECT_REFUSES_NULL(gss_cacgmm_guided);
    EXPECT_REFUSES_NULL(gss_cacgmm_fit);
    EXPECT_REFUSES_NULL(gss_cacgmm_predict);
    EXPECT_REFUSES_NULL(gss_masks_from_posteriors);
    EXPECT_REFUSES_NULL(gss_mvdr_souden);
    EXPECT_REFUSES_NULL(gss_mvdr_souden_ref);
    EXPECT_REFUSES_NULL(gss_mvdr_souden_segments);
    EXPECT_REFUSES_NULL(gss_lcmv_souden);
    EXPECT_REFUSES_NULL(gss_lcmv_masks_from_posteriors);
    EXPECT_REFUSES_NULL(gss_wpd_weights);
    EXPECT_REFUSES_NULL(gss_wpd_souden);
    EXPECT_REFUSES_NULL(gss_gev);
    EXPECT_REFUSES_NULL(gss_channel_scores);
    EXPECT_REFUSES_NULL(gss_select_channels);
    EXPECT_REFUSES_NULL(gss_posterior_activity);
    EXPECT_REFUSES_NULL(gss_layout_dtf_to_ftd);
    EXPECT_REFUSES_NULL(gss_layout_ftd_to_dtf);
    EXPECT_REFUSES_NULL(gss_layout_permute_f64);
    EXPECT_REFUSES_NULL(gss_last_ref_channel);
    EXPECT_REFUSES_NULL(gss_last_ref_channels);
    EXPECT_REFUSES_NULL(gss_last_wpe_zero_pivots);
    EXPECT_REFUSES_NULL(gss_last_wpd_zero_pivots);
    EXPECT_REFUSES_NULL(gss_last_segment_fallbacks);
    EXPECT_REFUSES_NULL(gss_last_lcmv_interferer);
    EXPECT_REFUSES_NULL(gss_last_lcmv_fallbacks);
    EXPECT_REFUSES_NULL(gss_last_selected_channels);
    EXPECT_REFUSES_NULL(gss_enhance_observation);
    EXPECT_REFUSES_NULL(gss_enhance_observation_pcm16);
    EXPECT_REFUSES_NULL(gss_enhance_observation_guided);
    EXPECT_REFUSES_NULL(gss_enhance_observation_segments);
    EXPECT_REFUSES_NULL(gss_enhance_observation_lcmv);
    EXPECT_REFUSES_NULL(gss_enhance_observation_wpd);
    EXPECT_REFUSES_NULL(gss_enhance_observation_activity);
    EXPECT_REFUSES_NULL(gss_enhance_observation_select);
    EXPECT_REFUSES_NULL(gss_enhance_observation_select_pcm16);
    EXPECT_REFUSES_NULL(gss_enhance_observation_targets);
    EXPECT_REFUSES_NULL(gss_enhance_observation_targets_pcm16);
    EXPECT_REFUSES_NULL(gss_enhance_observation_host);
    EXPECT_REFUSES_NULL(gss_selftest_mfma);

    std::printf(failures ? "%d check(s) failed\n" : "host paths clean (%d failures)\n", failures);
    return failures ? 1 : 0;
}
