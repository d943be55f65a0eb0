"""Which test reaches which kernel (a plain data module, like the spec table of the memory-contract tests; checked without a GPU
by tests/test_kernel_variants_host.py; derived by reading the launchers -- tools/kernel_trace_names.py reduces a kernel trace of
tests/test_gpu_kernel_variants.py to the names to compare with).

VARIANTS   one row per __global__ kernel instantiation of the SHIPPED library (build.py without --debug):
             kernel   the demangled name as `nm -C` prints it behind dvae::__device_stub__, template arguments included
                      (matched literally against the whole name);
             entry    the C-ABI entry point(s) whose launcher selects it;
             when     the argument condition, copied from the launcher;
             where    the launch site, file:line under disentangling-vae_amd/csrc/;
             test     node id of one GPU test that makes such a call, or None;
             reason   test is None: why no call of the shipped library can reach the kernel.
SWITCHES   every numeric threshold read in the launchers: (launcher, variable, threshold, where, last shape of one side, its
           test id, first shape of the other side, its test id -- a different id), or, where no call through the C-ABI can
           reach the flip, no shapes and no ids but a `reason`.
OPEN_SWITCHES  thresholds read in the launchers without such a pair: empty, and held empty by the host test -- a newly found
           threshold goes into SWITCHES with its pair.
TRIP_CLASSES  per persistent (grid-capped) kernel family: grid size and trips of workgroup b as Python expressions of the image
           count N copied from the launcher and the kernel's loop, the depth of its software pipeline (units in flight per
           workgroup; 1 = the loop holds one unit at a time), the smallest N that reaches the kernel, and the tests that sit
           at each required trip-count class:
             uniform t  (every workgroup makes t trips) for each t from the kernel's minimum to depth + 1,
             one uniform odd and one uniform even count above the depth,
             one mixed launch (workgroups of t + 1 and of t trips side by side);
           `unreachable` names the uniform counts that no image count gives.  The host test evaluates the expressions at the N
           of each named id and asserts that the class claimed is the class obtained.
"""
from collections import namedtuple

Variant = namedtuple("Variant", "kernel entry when where test reason")
Switch = namedtuple("Switch", "launcher variable threshold where below below_test above above_test reason")
TripFamily = namedtuple("TripFamily", "family where grid trips depth n_from cases unreachable")

K = "tests/test_gpu_kernels.py::"
V = "tests/test_gpu_kernel_variants.py::"
B = "tests/test_gpu_bench_sizes.py::"
FC = "tests/test_gpu_fused_core.py::"
MB = "tests/test_gpu_mask_bits.py::"
U8 = "tests/test_gpu_uint8_input.py::"
MC = "tests/test_gpu_memory_contract.py::test_memory_contract"
WL = "tests/test_gpu_wide_latent.py::"
T = "tests/test_gpu_trip_counts.py::"

_DEBUG_ONLY = ("the wave-specialised kernel takes every shape this one covers; the launcher falls through to it only with %s=0, "
               "an environment switch that exists in --debug builds only (common.h: env_off() is constant false)")
_SMALL_ONLY = ("use_small() (linear.hip:559) returns true only for the forward with K % 4 == 0 unless DVAE_GEMM_SMALL is set, "
               "which --debug builds only read")


def _v(kernel, entry, when, where, test=None, reason=None):
    return Variant(kernel, entry, when, where, test, reason)


VARIANTS = [
    # ---- adam.hip
    _v("k_adam", "dvae_adam_step", "always; one launch per ADAM_MAX_T = 64 tensors", "adam.hip:91", V + "test_adam_at_the_table_split[65]"),
    # ---- conv_down_dma.hip (launch_down_mfma32 -> launch_down_mfma32_dma: 32 <-> 32 channels, NHWC, Hs in {16, 8})
    _v("k_down32dma<16, false>", "dvae_conv4s2_fwd, dvae_conv32_down", "Hs == 16, no mask", "conv_down_dma.hip:232", V + "test_conv32_at_the_persistent_grid_switch[64-16]"),
    _v("k_down32dma<16, true>", "dvae_convT4s2_dgrad, dvae_conv32_down", "Hs == 16, mask", "conv_down_dma.hip:231", V + "test_conv32_at_the_persistent_grid_switch[65-16]"),
    _v("k_down32dma<8, false>", "dvae_conv4s2_fwd, dvae_conv32_down", "Hs == 8, no mask", "conv_down_dma.hip:232", V + "test_conv32_at_the_persistent_grid_switch[256-8]"),
    _v("k_down32dma<8, true>", "dvae_convT4s2_dgrad, dvae_conv32_down", "Hs == 8, mask", "conv_down_dma.hip:231", V + "test_conv32_at_the_persistent_grid_switch[257-8]"),
    # ---- conv_generic.hip
    _v("k_chansum", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "generic geometry, db != NULL, fewer than 2 position chunks", "conv_generic.hip:399", V + "test_generic_wgrad_at_the_chunk_switches[7]"),
    _v("k_relayout", "dvae_relayout", "always", "conv_generic.hip:424", K + "test_relayout"),
    _v("k_up_generic", "dvae_convT4s2_fwd, dvae_conv4s2_dgrad", "no tuned kernel applies or DVAE_FORCE_GENERIC=1", "conv_generic.hip:370", K + "test_convT_fwd_dgrad_wgrad[3-16-32-1-1-True]"),
    _v("k_up_thin_px<1>", "dvae_convT4s2_fwd, dvae_conv4s2_dgrad", "Cs == 32, Cb == 1, small NHWC, not 64x64", "conv_generic.hip:364", K + "test_thin_ends_at_any_size_match_the_plain_generic_kernels[3-1-32]"),
    _v("k_up_thin_px<3>", "dvae_convT4s2_fwd, dvae_conv4s2_dgrad", "Cs == 32, Cb == 3, small NHWC, not 64x64", "conv_generic.hip:365", K + "test_thin_ends_at_any_size_match_the_plain_generic_kernels[5-3-32]"),
    _v("k_down_generic", "dvae_conv4s2_fwd, dvae_convT4s2_dgrad", "no tuned kernel applies or DVAE_FORCE_GENERIC=1", "conv_generic.hip:351", K + "test_conv_fwd_dgrad_wgrad[3-32-32-1-True]"),
    _v("k_down_thin_px<1>", "dvae_conv4s2_fwd, dvae_convT4s2_dgrad", "Cs == 32, Cb == 1, NCHW -> NHWC, not 64x64", "conv_generic.hip:345", K + "test_thin_ends_at_any_size_match_the_plain_generic_kernels[3-1-32]"),
    _v("k_down_thin_px<3>", "dvae_conv4s2_fwd, dvae_convT4s2_dgrad", "Cs == 32, Cb == 3, NCHW -> NHWC, not 64x64", "conv_generic.hip:346", K + "test_thin_ends_at_any_size_match_the_plain_generic_kernels[5-3-32]"),
    _v("k_wgrad_generic", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "generic geometry, N * Hs * Ws / 1024 < 2 or no workspace", "conv_generic.hip:395", V + "test_generic_wgrad_at_the_chunk_switches[7]"),
    _v("k_wgrad_generic_fin", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "generic geometry, N * Hs * Ws / 1024 >= 2, workspace", "conv_generic.hip:390", V + "test_generic_wgrad_at_the_chunk_switches[8]"),
    _v("k_wgrad_generic_part", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "generic geometry, N * Hs * Ws / 1024 >= 2, workspace", "conv_generic.hip:386", V + "test_generic_wgrad_at_the_chunk_switches[8]"),
    # ---- conv_mfma.hip
    _v("k_up32<16, false>", "dvae_convT4s2_fwd, dvae_conv32_up", "Hs == 16, no mask, after launch_up_mfma32_ws declined", "conv_mfma.hip:414", None, _DEBUG_ONLY % "DVAE_UP_WS"),
    _v("k_up32<16, true>", "dvae_conv4s2_dgrad, dvae_conv32_up", "Hs == 16, mask, after launch_up_mfma32_ws declined", "conv_mfma.hip:413", None, _DEBUG_ONLY % "DVAE_UP_WS"),
    _v("k_up32<8, false>", "dvae_convT4s2_fwd, dvae_conv32_up", "Hs == 8, no mask, after launch_up_mfma32_ws declined", "conv_mfma.hip:414", None, _DEBUG_ONLY % "DVAE_UP_WS"),
    _v("k_up32<8, true>", "dvae_conv4s2_dgrad, dvae_conv32_up", "Hs == 8, mask, after launch_up_mfma32_ws declined", "conv_mfma.hip:413", None, _DEBUG_ONLY % "DVAE_UP_WS"),
    _v("k_up32<4, false>", "dvae_convT4s2_fwd, dvae_conv32_up", "Hs == 4, no mask (small side NHWC or NCHW)", "conv_mfma.hip:414", V + "test_conv32_at_the_persistent_grid_switch[1024-4]"),
    _v("k_up32<4, true>", "dvae_conv4s2_dgrad, dvae_conv32_up", "Hs == 4, mask", "conv_mfma.hip:413", V + "test_conv32_at_the_persistent_grid_switch[1025-4]"),
    _v("k_down32<4, false>", "dvae_conv4s2_fwd, dvae_conv32_down", "Hs == 4, no mask (output NHWC or NCHW)", "conv_mfma.hip:396", V + "test_conv32_at_the_persistent_grid_switch[1024-4]"),
    _v("k_down32<4, true>", "dvae_convT4s2_dgrad, dvae_conv32_down", "Hs == 4, mask", "conv_mfma.hip:395", V + "test_conv32_at_the_persistent_grid_switch[1025-4]"),
    _v("k_wgrad32<16>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "Hs == 16 with the small side NCHW or DVAE_WGRAD_WS=0", "conv_mfma.hip:433", None,
       "run_wgrad (capi.hip:60) passes small_nchw = 1 for Hs == 4 only, and " + _DEBUG_ONLY % "DVAE_WGRAD_WS"),
    _v("k_wgrad32<8>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "Hs == 8 with the small side NCHW or DVAE_WGRAD_WS=0", "conv_mfma.hip:433", None,
       "run_wgrad (capi.hip:60) passes small_nchw = 1 for Hs == 4 only, and " + _DEBUG_ONLY % "DVAE_WGRAD_WS"),
    _v("k_wgrad32<4>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "Hs == 4 (small side NHWC or NCHW)", "conv_mfma.hip:433", V + "test_wgrad32_at_the_reduction_form_switch[767-4-True-False]"),
    _v("k_wgrad32_reduce<false>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "32 <-> 32 channels, N < WGR_LEAN_MIN_IMAGES = 768", "conv_mfma.hip:375", V + "test_wgrad32_at_the_reduction_form_switch[767-8-False-False]"),
    _v("k_wgrad32_reduce<true>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "32 <-> 32 channels, N >= 768", "conv_mfma.hip:373", V + "test_wgrad32_at_the_reduction_form_switch[768-8-False-False]"),
    # ---- conv_thin.hip (C = 1 / 3 <-> 32 channels, 64x64 <-> 32x32)
    _v("k_up_thin<1, false, float>", "dvae_convT4s2_fwd", "Cb == 1, NHWC -> NCHW, no mask, act not leaky, aligned", "conv_thin.hip:697", K + "test_convT_fwd_dgrad_wgrad[3-32-1-0-3-False]"),
    _v("k_up_thin<1, true, float>", "dvae_convT4s2_sigmoid_recon_fwd", "Cb == 1", "conv_thin.hip:709", K + "test_convT_sigmoid_recon_fused[3-1-32-gaussian-False]"),
    _v("k_up_thin<1, true, unsigned char>", "dvae_convT4s2_sigmoid_recon_fwd_u8", "Cb == 1", "conv_thin.hip:734", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[3-1]"),
    _v("k_up_thin<3, false, float>", "dvae_convT4s2_fwd", "Cb == 3, NHWC -> NCHW, no mask, act not leaky, aligned", "conv_thin.hip:698", K + "test_convT_fwd_dgrad_wgrad[5-32-3-0-3-False]"),
    _v("k_up_thin<3, true, float>", "dvae_convT4s2_sigmoid_recon_fwd", "Cb == 3", "conv_thin.hip:710", K + "test_convT_sigmoid_recon_fused[5-3-32-bernoulli-False]"),
    _v("k_up_thin<3, true, unsigned char>", "dvae_convT4s2_sigmoid_recon_fwd_u8", "Cb == 3", "conv_thin.hip:735", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[5-3]"),
    _v("k_down_thin<1, 0, float>", "dvae_conv4s2_fwd", "Cb == 1, N < 192, no mask", "conv_thin.hip:684", V + "test_thin_ends_at_the_wave_specialised_switch[191-1]"),
    _v("k_down_thin<1, 0, unsigned char>", "dvae_conv4s2_fwd_u8", "Cin == 1", "conv_thin.hip:721", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[3-1]"),
    _v("k_down_thin<1, 1, float>", "dvae_convT4s2_dgrad", "Cb == 1, fp32 mask (any N)", "conv_thin.hip:684", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_down_thin<1, 2, float>", "dvae_convT3_dgrad_bits", "Cout == 1, N < 192", "conv_thin.hip:684", V + "test_thin_ends_at_the_wave_specialised_switch[191-1]"),
    _v("k_down_thin<1, 3, float>", "dvae_conv1_fwd_bits", "Cin == 1, fp32 input, N < 192", "conv_thin.hip:684", V + "test_thin_ends_at_the_wave_specialised_switch[191-1]"),
    _v("k_down_thin<1, 3, unsigned char>", "dvae_conv1_fwd_bits", "Cin == 1, uint8 input", "conv_thin.hip:721", MB + "test_conv1_forward_emits_the_bit_plane[9-1-True]"),
    _v("k_down_thin<3, 0, float>", "dvae_conv4s2_fwd", "Cb == 3, N < 192, no mask", "conv_thin.hip:686", V + "test_thin_ends_at_the_wave_specialised_switch[191-3]"),
    _v("k_down_thin<3, 0, unsigned char>", "dvae_conv4s2_fwd_u8", "Cin == 3", "conv_thin.hip:722", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[5-3]"),
    _v("k_down_thin<3, 1, float>", "dvae_convT4s2_dgrad", "Cb == 3, fp32 mask (any N)", "conv_thin.hip:686", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    _v("k_down_thin<3, 2, float>", "dvae_convT3_dgrad_bits", "Cout == 3, N < 192", "conv_thin.hip:686", V + "test_thin_ends_at_the_wave_specialised_switch[191-3]"),
    _v("k_down_thin<3, 3, float>", "dvae_conv1_fwd_bits", "Cin == 3, fp32 input, N < 192", "conv_thin.hip:686", V + "test_thin_ends_at_the_wave_specialised_switch[191-3]"),
    _v("k_down_thin<3, 3, unsigned char>", "dvae_conv1_fwd_bits", "Cin == 3, uint8 input", "conv_thin.hip:722", MB + "test_conv1_forward_emits_the_bit_plane[520-3-True]"),
    _v("k_up_thin_pk<1, false, float>", "dvae_convT3_fwd_staged", "C == 1, no target", "conv_thin.hip:548", FC + "test_convT3_forward_on_staged_pair_records[3-1]"),
    _v("k_up_thin_pk<1, true, float>", "dvae_convT3_fwd_staged", "C == 1, fp32 target", "conv_thin.hip:550", FC + "test_convT3_forward_on_staged_pair_records[3-1]"),
    _v("k_up_thin_pk<1, true, unsigned char>", "dvae_convT3_fwd_staged", "C == 1, uint8 target", "conv_thin.hip:549", FC + "test_convT3_forward_on_staged_pair_records[3-1]"),
    _v("k_up_thin_pk<3, false, float>", "dvae_convT3_fwd_staged", "C == 3, no target, recon / g / fp32 target not 16-byte or uint8 target not 4-byte aligned (k_up_thin_mm declines)", "conv_thin.hip:548", V + "test_convT3_staged_falls_back_to_the_packed_fma_kernel"),
    _v("k_up_thin_pk<3, true, float>", "dvae_convT3_fwd_staged", "C == 3, fp32 target, recon / g / fp32 target not 16-byte or uint8 target not 4-byte aligned (k_up_thin_mm declines)", "conv_thin.hip:550", V + "test_convT3_staged_falls_back_to_the_packed_fma_kernel"),
    _v("k_up_thin_pk<3, true, unsigned char>", "dvae_convT3_fwd_staged", "C == 3, uint8 target, recon / g / fp32 target not 16-byte or uint8 target not 4-byte aligned (k_up_thin_mm declines)", "conv_thin.hip:549", V + "test_convT3_staged_falls_back_to_the_packed_fma_kernel"),
    _v("k_wgrad_thin<1, float>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "Cb == 1, N < 192", "conv_thin.hip:750", V + "test_thin_ends_at_the_wave_specialised_switch[191-1]"),
    _v("k_wgrad_thin<1, unsigned char>", "dvae_conv4s2_wgrad_u8", "Cin == 1", "conv_thin.hip:750", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[3-1]"),
    _v("k_wgrad_thin<3, float>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "Cb == 3, N < 192", "conv_thin.hip:750", V + "test_thin_ends_at_the_wave_specialised_switch[191-3]"),
    _v("k_wgrad_thin<3, unsigned char>", "dvae_conv4s2_wgrad_u8", "Cin == 3", "conv_thin.hip:750", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[5-3]"),
    _v("k_wgrad_thin_reduce<1>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad, dvae_conv4s2_wgrad_u8", "Cb == 1, behind either partial kernel", "conv_thin.hip:743", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_wgrad_thin_reduce<3>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad, dvae_conv4s2_wgrad_u8", "Cb == 3, behind either partial kernel", "conv_thin.hip:743", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    # ---- conv_thin_ws.hip (N >= 192, 16-byte aligned buffers)
    _v("k_down_thin_ws<1, 0, 0>", "dvae_conv4s2_fwd", "Cb == 1, N >= 192, no mask", "conv_thin_ws.hip:368", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_down_thin_ws<1, 2, 0>", "dvae_convT3_dgrad_bits", "Cout == 1, N >= 192", "conv_thin_ws.hip:368", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_down_thin_ws<1, 3, 0>", "dvae_conv1_fwd_bits", "Cin == 1, fp32 input, N >= 192", "conv_thin_ws.hip:368", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_down_thin_ws<3, 0, 0>", "dvae_conv4s2_fwd", "Cb == 3, N >= 192, no mask", "conv_thin_ws.hip:370", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    _v("k_down_thin_ws<3, 2, 0>", "dvae_convT3_dgrad_bits", "Cout == 3, N >= 192", "conv_thin_ws.hip:370", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    _v("k_down_thin_ws<3, 3, 0>", "dvae_conv1_fwd_bits", "Cin == 3, fp32 input, N >= 192", "conv_thin_ws.hip:370", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    _v("k_wgrad_thin_ws<1, false, 0>", "dvae_conv4s2_wgrad", "Cb == 1, N >= 192, bias from the 32-channel side", "conv_thin_ws.hip:640", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_wgrad_thin_ws<1, true, 0>", "dvae_convT4s2_wgrad", "Cb == 1, N >= 192, bias from the thin side", "conv_thin_ws.hip:640", V + "test_thin_ends_at_the_wave_specialised_switch[192-1]"),
    _v("k_wgrad_thin_ws<3, false, 0>", "dvae_conv4s2_wgrad", "Cb == 3, N >= 192, bias from the 32-channel side", "conv_thin_ws.hip:641", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    _v("k_wgrad_thin_ws<3, true, 0>", "dvae_convT4s2_wgrad", "Cb == 3, N >= 192, bias from the thin side", "conv_thin_ws.hip:641", V + "test_thin_ends_at_the_wave_specialised_switch[192-3]"),
    # ---- conv_up_thin_mm.hip (dvae_convT3_fwd_staged, C == 3, 16-byte aligned buffers)
    _v("k_up_thin_mm<false, 0, float>", "dvae_convT3_fwd_staged", "C == 3, no target", "conv_up_thin_mm.hip:288", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    _v("k_up_thin_mm<true, 0, float>", "dvae_convT3_fwd_staged", "C == 3, fp32 target, bernoulli", "conv_up_thin_mm.hip:294", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    _v("k_up_thin_mm<true, 0, unsigned char>", "dvae_convT3_fwd_staged", "C == 3, uint8 target, bernoulli", "conv_up_thin_mm.hip:290", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    _v("k_up_thin_mm<true, 1, float>", "dvae_convT3_fwd_staged", "C == 3, fp32 target, gaussian", "conv_up_thin_mm.hip:295", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    _v("k_up_thin_mm<true, 1, unsigned char>", "dvae_convT3_fwd_staged", "C == 3, uint8 target, gaussian", "conv_up_thin_mm.hip:291", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    _v("k_up_thin_mm<true, 2, float>", "dvae_convT3_fwd_staged", "C == 3, fp32 target, laplace", "conv_up_thin_mm.hip:296", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    _v("k_up_thin_mm<true, 2, unsigned char>", "dvae_convT3_fwd_staged", "C == 3, uint8 target, laplace", "conv_up_thin_mm.hip:292", FC + "test_convT3_forward_on_staged_pair_records[3-3]"),
    # ---- conv_up_ws.hip (32 <-> 32 channels, NHWC, Hs in {16, 8})
    _v("k_up32ws<16, 0, false>", "dvae_convT4s2_fwd, dvae_conv32_up", "Hs == 16, no mask", "conv_up_ws.hip:374", V + "test_conv32_at_the_persistent_grid_switch[64-16]"),
    _v("k_up32ws<16, 0, true>", "dvae_conv32_up_bits", "out_bits != NULL (ReLU forward that emits the bit plane)", "conv_up_ws.hip:369", MB + "test_conv32_up_bits_forward_and_input_gradient[300]"),
    _v("k_up32ws<16, 1, false>", "dvae_conv4s2_dgrad, dvae_conv32_up", "Hs == 16, fp32 mask", "conv_up_ws.hip:372", V + "test_conv32_at_the_persistent_grid_switch[65-16]"),
    _v("k_up32ws<16, 2, false>", "dvae_conv32_up_bits", "mask_bits != NULL", "conv_up_ws.hip:366", MB + "test_conv32_up_bits_forward_and_input_gradient[300]"),
    _v("k_up32ws<8, 0, false>", "dvae_convT4s2_fwd, dvae_conv32_up", "Hs == 8, no mask", "conv_up_ws.hip:374", V + "test_conv32_at_the_persistent_grid_switch[256-8]"),
    _v("k_up32ws<8, 1, false>", "dvae_conv4s2_dgrad, dvae_conv32_up", "Hs == 8, fp32 mask", "conv_up_ws.hip:372", V + "test_conv32_at_the_persistent_grid_switch[257-8]"),
    # ---- conv_wgrad_ws.hip
    _v("k_wgrad32ws<16>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "32 <-> 32 channels, NHWC, Hs == 16", "conv_wgrad_ws.hip:319", V + "test_conv_wgrad32_at_the_grid_cap[129-16]"),
    _v("k_wgrad32ws<8>", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad", "32 <-> 32 channels, NHWC, Hs == 8", "conv_wgrad_ws.hip:319", V + "test_conv_wgrad32_at_the_grid_cap[129-8]"),
    # ---- gemm_dma.hip (try_gdma: Kc >= 256, N >= 128, aligned; tile from ceil(M / tile) * ceil(N / 64))
    _v("k_gdma<128, 64, 32, 4, 1, false, 0>", "dvae_linear_fwd", "ceil(M / 128) * cols64 >= 224", "gemm_dma.hip:508", V + "test_discriminator_linear_at_the_tile_switches[1665]"),
    _v("k_gdma<128, 64, 32, 4, 1, true, 0>", "dvae_linear_dgrad", "ceil(M / 128) * cols64 >= 224", "gemm_dma.hip:508", V + "test_discriminator_linear_at_the_tile_switches[1665]"),
    _v("k_gdma<32, 32, 64, 3, 4, false, 0>", "dvae_linear_fwd", "ceil(M / 64) * cols64 < 192", "gemm_dma.hip:510", V + "test_discriminator_linear_at_the_tile_switches[704]"),
    _v("k_gdma<32, 32, 64, 3, 4, true, 0>", "dvae_linear_dgrad", "ceil(M / 64) * cols64 < 192", "gemm_dma.hip:510", V + "test_discriminator_linear_at_the_tile_switches[704]"),
    _v("k_gdma<64, 64, 64, 3, 1, false, 0>", "dvae_linear_fwd", "ceil(M / 64) * cols64 >= 192, ceil(M / 128) * cols64 < 224", "gemm_dma.hip:509", V + "test_discriminator_linear_at_the_tile_switches[705]"),
    _v("k_gdma<64, 64, 64, 3, 1, true, 0>", "dvae_linear_dgrad", "ceil(M / 64) * cols64 >= 192, ceil(M / 128) * cols64 < 224", "gemm_dma.hip:509", V + "test_discriminator_linear_at_the_tile_switches[1664]"),
    _v("k_gdma_wg<64, 3>", "dvae_linear_wgrad", "M >= 64, N % 4 == K % 4 == 0, >= 128 output tiles of 64x64", "gemm_dma.hip:527", V + "test_discriminator_linear_at_the_tile_switches[64]"),
    # ---- latent_wide.hip (D > DVAE_MAX_D = 16)
    _v("k_tcw_joint", "dvae_btcvae_fwd", "D > 16", "latent_wide.hip:211", WL + "test_btcvae_fwd_bwd_wide[4-100-True-17]"),
    _v("k_kl_cols_wide", "dvae_reparam_kl_fwd", "D > 16, kl_dim != NULL", "latent_wide.hip:202", WL + "test_reparam_kl_wide[2-17]"),
    _v("k_reparam_wide", "dvae_reparam_kl_fwd", "D > 16", "latent_wide.hip:199", WL + "test_reparam_kl_wide[2-17]"),
    _v("k_tcw_bwd_cols", "dvae_btcvae_bwd", "D > 16", "latent_wide.hip:227", WL + "test_btcvae_fwd_bwd_wide[4-100-True-17]"),
    _v("k_tcw_bwd_rows", "dvae_btcvae_bwd", "D > 16", "latent_wide.hip:224", WL + "test_btcvae_fwd_bwd_wide[4-100-True-17]"),
    _v("k_tcw_rowstats", "dvae_btcvae_fwd", "D > 16", "latent_wide.hip:213", WL + "test_btcvae_fwd_bwd_wide[4-100-True-17]"),
    # ---- linear.hip (try_fc32: contraction <= 512 and < 512 output tiles of 64x64; KP = the contraction rounded up)
    _v("k_fc32<128, false, 0>", "dvae_linear_fwd", "64 < K <= 128, K % 4 == 0", "linear.hip:429", V + "test_linear_at_the_contraction_length_switches[128]"),
    _v("k_fc32<128, true, 0>", "dvae_linear_dgrad", "64 < N <= 128, N % 4 == K % 4 == 0", "linear.hip:429", V + "test_linear_at_the_contraction_length_switches[68]"),
    _v("k_fc32<128, true, 2>", "dvae_linear_dgrad", "64 < N <= 128, K % 4 != 0", "linear.hip:429", V + "test_linear_dgrad_into_a_narrow_unaligned_output[128]"),
    _v("k_fc32<256, false, 0>", "dvae_linear_fwd", "128 < K <= 256, K % 4 == 0", "linear.hip:430", V + "test_linear_at_the_contraction_length_switches[132]"),
    _v("k_fc32<256, true, 0>", "dvae_linear_dgrad", "128 < N <= 256, N % 4 == K % 4 == 0", "linear.hip:430", V + "test_linear_at_the_contraction_length_switches[256]"),
    _v("k_fc32<256, true, 2>", "dvae_linear_dgrad", "128 < N <= 256, K % 4 != 0", "linear.hip:430", V + "test_linear_dgrad_into_a_narrow_unaligned_output[256]"),
    _v("k_fc32<32, false, 0>", "dvae_linear_fwd", "K <= 32, K % 4 == 0, aligned", "linear.hip:427", V + "test_linear_at_the_contraction_length_switches[32]"),
    _v("k_fc32<32, false, 1>", "dvae_linear_fwd", "K <= 32, K % 4 != 0 or unaligned", "linear.hip:416", V + "test_linear_dgrad_into_a_narrow_unaligned_output[32]"),
    _v("k_fc32<32, true, 0>", "dvae_linear_dgrad", "N <= 32, N % 4 == K % 4 == 0", "linear.hip:427", V + "test_linear_at_the_contraction_length_switches[32]"),
    _v("k_fc32<32, true, 2>", "dvae_linear_dgrad", "N <= 32, K % 4 != 0", "linear.hip:427", V + "test_linear_dgrad_into_a_narrow_unaligned_output[32]"),
    _v("k_fc32<512, false, 0>", "dvae_linear_fwd", "256 < K <= 512, K % 4 == 0", "linear.hip:431", V + "test_linear_at_the_contraction_length_switches[260]"),
    _v("k_fc32<512, true, 0>", "dvae_linear_dgrad", "256 < N <= 512, N % 4 == K % 4 == 0", "linear.hip:431", V + "test_linear_at_the_contraction_length_switches[512]"),
    _v("k_fc32<512, true, 2>", "dvae_linear_dgrad", "256 < N <= 512, K % 4 != 0", "linear.hip:431", V + "test_linear_dgrad_into_a_narrow_unaligned_output[512]"),
    _v("k_fc32<64, false, 0>", "dvae_linear_fwd", "32 < K <= 64, K % 4 == 0", "linear.hip:428", V + "test_linear_at_the_contraction_length_switches[36]"),
    _v("k_fc32<64, true, 0>", "dvae_linear_dgrad", "32 < N <= 64, N % 4 == K % 4 == 0", "linear.hip:428", V + "test_linear_at_the_contraction_length_switches[64]"),
    _v("k_fc32<64, true, 2>", "dvae_linear_dgrad", "32 < N <= 64, K % 4 != 0", "linear.hip:428", V + "test_linear_dgrad_into_a_narrow_unaligned_output[64]"),
    _v("k_gemm<false, true>", "dvae_linear_wgrad", "M > 4096 or >= 512 output tiles, and not k_gdma_wg", "linear.hip:721", V + "test_linear_wgrad_at_the_batch_switches[4100]"),
    _v("k_gemm<true, false>", "dvae_linear_fwd", "no other forward kernel applies (>= 512 output tiles with K < 256; K % 4 != 0 above 32)", "linear.hip:643", V + "test_linear_at_the_output_tile_count_switch[2048-64-1024-parts1]"),
    _v("k_gemm<true, true>", "dvae_linear_dgrad", "no other input-gradient kernel applies (N > 512 into K < 128 columns; >= 512 output tiles)", "linear.hip:682", V + "test_linear_at_the_output_tile_count_switch[2048-1024-64-parts3]"),
    _v("k_fcw32<256>", "dvae_linear_wgrad", "64 < M <= 4096, < 512 output tiles", "linear.hip:549", V + "test_linear_wgrad_at_the_batch_switches[65]"),
    _v("k_fcw32<64>", "dvae_linear_wgrad", "M <= 64, < 512 output tiles", "linear.hip:541", V + "test_linear_wgrad_at_the_batch_switches[64]"),
    _v("k_gemm32<false, false>", "dvae_linear_fwd, dvae_linear_dgrad, dvae_linear_wgrad", "use_small() and an unaligned contraction", "linear.hip:635", None, _SMALL_ONLY),
    _v("k_gemm32<true, false>", "dvae_linear_dgrad", "use_small(), N % 4 == 0", "linear.hip:671", None, _SMALL_ONLY),
    _v("k_gemm32<true, true>", "dvae_linear_fwd", "K > 512, K % 4 == 0, < 192 output tiles, N < 128 (not k_gdma)", "linear.hip:632", V + "test_linear_outside_the_lds_resident_kernels[40-1000-36]"),
    _v("k_splitk_reduce", "dvae_linear_wgrad", "k_gemm<false, true> with a workspace and S > 1 contraction slices", "linear.hip:734", V + "test_linear_wgrad_at_the_batch_switches[4100]"),
    _v("k_splitk_epilogue", "dvae_linear_fwd, dvae_linear_dgrad", "k_gemm<true, *> with a workspace and S > 1 contraction slices", "linear.hip:654", V + "test_linear_outside_the_lds_resident_kernels[40-301-36]"),
    # ---- linear_grouped.hip
    _v("k_fcw_grouped<128>", "dvae_linear_wgrad_grouped", "64 < max M <= 128", "linear_grouped.hip:166", V + "test_linear_wgrad_grouped_past_its_slab_switches[65]"),
    _v("k_fcw_grouped<256>", "dvae_linear_wgrad_grouped", "max M > 128", "linear_grouped.hip:167", V + "test_linear_wgrad_grouped_past_its_slab_switches[129]"),
    _v("k_fcw_grouped<64>", "dvae_linear_wgrad_grouped", "max M <= 64", "linear_grouped.hip:165", K + "test_linear_wgrad_grouped[64]"),
    # ---- linear_narrow.hip
    _v("k_narrow_out_fwd", "dvae_linear_fwd", "N <= 8, K >= 256, K % 4 == 0, aligned", "linear_narrow.hip:89", V + "test_narrow_output_linear_at_its_minimum_contraction[256]"),
    _v("k_narrow_out_dgrad", "dvae_linear_dgrad", "N <= 8, K >= 256, K % 4 == 0, aligned", "linear_narrow.hip:102", V + "test_narrow_output_linear_at_its_minimum_contraction[256]"),
    # ---- loglik.hip
    _v("k_iw_loglik", "dvae_iw_loglik", "always", "loglik.hip:177", "tests/test_gpu_loglik.py::test_log_likelihood_vs_fp64_restatement[img0-10-37-64-bernoulli-False]"),
    _v("k_recon_rows", "dvae_recon_rows", "always", "loglik.hip:158", "tests/test_gpu_loglik.py::test_recon_rows_vs_fp64_oracle[bernoulli-False-img0-1]"),
    _v("k_recon_rows_finish", "dvae_recon_rows", "more than one slice of a row", "loglik.hip:163", "tests/test_gpu_loglik.py::test_recon_rows_vs_fp64_oracle[bernoulli-False-img1-1]"),
    # ---- loss.hip
    _v("k_add", "dvae_add", "always", "loss.hip:861", FC + "test_event_slots_order_a_late_consumer_after_marked_work"),
    _v("k_axpby", "dvae_axpby", "always", "loss.hip:868", K + "test_data_parallel_glue_kernels"),
    _v("k_set_coef", "dvae_set_coef", "always", "loss.hip:854", MC + "[set_coef]"),
    _v("k_loss_pack", "dvae_loss_pack", "always", "loss.hip:793", K + "test_loss_epilogue_equals_pack_then_finalize[0-8]"),
    _v("k_u8_to_f32", "dvae_u8_to_f32", "always", "loss.hip:846", U8 + "test_u8_to_f32_is_totensor"),
    _v("k_btcvae_fwd<0>", "dvae_btcvae_fwd", "D <= 16, D != 10", "loss.hip:756", V + "test_btcvae_bwd_at_the_row_switch[513-6-True]"),
    _v("k_btcvae_fwd<10>", "dvae_btcvae_fwd", "D == 10", "loss.hip:756", V + "test_btcvae_bwd_at_the_row_switch[513-10-True]"),
    _v("k_recon_loss", "dvae_recon_loss, dvae_convT4s2_sigmoid_recon_fwd (two-pass shapes)", "always", "loss.hip:734", K + "test_recon_loss[bernoulli]"),
    _v("k_reduce_sum", "dvae_reduce_sum", "always", "loss.hip:839", MC + "[reduce_sum-n7]"),
    _v("k_swap_outer", "dvae_swap_outer", "always", "loss.hip:874", K + "test_data_parallel_glue_kernels"),
    _v("k_btcvae_prep", "dvae_btcvae_fwd", "always", "loss.hip:753", V + "test_btcvae_bwd_at_the_row_switch[512-10-True]"),
    _v("k_disc_losses", "dvae_disc_losses", "always", "loss.hip:786", K + "test_permute_dims_and_disc_losses"),
    _v("k_sigmoid_bwd", "dvae_sigmoid_bwd", "always", "loss.hip:826", K + "test_recon_loss[bernoulli]"),
    _v("k_permute_dims", "dvae_permute_dims", "always", "loss.hip:779", K + "test_permute_dims_and_disc_losses"),
    _v("k_btcvae_bwd_wg<0>", "dvae_btcvae_bwd", "Bl <= 512, D <= 16, D != 10", "loss.hip:769", V + "test_btcvae_bwd_at_the_row_switch[512-6-True]"),
    _v("k_btcvae_bwd_wg<10>", "dvae_btcvae_bwd", "Bl <= 512, D == 10", "loss.hip:769", V + "test_btcvae_bwd_at_the_row_switch[512-10-True]"),
    _v("k_kl_normal_bwd", "dvae_kl_normal_bwd", "always", "loss.hip:833", MC + "[kl_normal_bwd-B7-D1]"),
    _v("k_loss_epilogue", "dvae_loss_epilogue", "always", "loss.hip:812", K + "test_loss_epilogue_equals_pack_then_finalize[0-8]"),
    _v("k_loss_finalize", "dvae_loss_finalize", "always", "loss.hip:819", K + "test_loss_epilogue_equals_pack_then_finalize[0-8]"),
    _v("k_reparam_kl_bwd", "dvae_reparam_kl_bwd", "always", "loss.hip:726", K + "test_reparam_kl[8]"),
    _v("k_reparam_kl_fwd", "dvae_reparam_kl_fwd", "D <= 16", "loss.hip:712", V + "test_reparam_kl_at_the_partial_block_switches[257]"),
    _v("k_btcvae_bwd_cols<0>", "dvae_btcvae_bwd", "Bl > 512, D <= 16, D != 10", "loss.hip:773", V + "test_btcvae_bwd_at_the_row_switch[513-6-True]"),
    _v("k_btcvae_bwd_cols<10>", "dvae_btcvae_bwd", "Bl > 512, D == 10", "loss.hip:773", V + "test_btcvae_bwd_at_the_row_switch[513-10-True]"),
    _v("k_btcvae_bwd_rows<0>", "dvae_btcvae_bwd", "Bl > 512, D <= 16, D != 10", "loss.hip:772", V + "test_btcvae_bwd_at_the_row_switch[513-6-True]"),
    _v("k_btcvae_bwd_rows<10>", "dvae_btcvae_bwd", "Bl > 512, D == 10", "loss.hip:772", V + "test_btcvae_bwd_at_the_row_switch[513-10-True]"),
    _v("k_reparam_kl_finish", "dvae_reparam_kl_fwd, dvae_kl_finish", "kl_dim and coef given", "loss.hip:715", V + "test_reparam_kl_at_the_partial_block_switches[257]"),
    # ---- metrics.hip
    _v("k_entropy_lse", "dvae_latent_entropy", "always", "metrics.hip:114", "tests/test_gpu_metrics.py::test_entropy_kernel_vs_oracle[17-3-5]"),
    _v("k_entropy_prep", "dvae_latent_entropy", "always", "metrics.hip:112", "tests/test_gpu_metrics.py::test_entropy_kernel_vs_oracle[17-3-5]"),
    _v("k_entropy_finish", "dvae_latent_entropy", "always", "metrics.hip:116", "tests/test_gpu_metrics.py::test_entropy_kernel_vs_oracle[17-3-5]"),
    # ---- stage.hip, viz.hip
    _v("k_stage_weights", "dvae_stage_weights", "at least one image or the coefficients", "stage.hip:137", FC + "test_stage_weights_layouts_and_coefficients"),
    _v("k_image_grid_u8", "dvae_image_grid_u8", "always", "viz.hip:111", "tests/test_gpu_visualize.py::test_grid_kernel_matches_make_grid[3-32]"),
    # ---- fc_chain.hip (<DEPTH = 8, KS = 2, RG, CONV>: RG = 1 up to 1024 rows, 2 above; CONV = the conv ends in the launch)
    _v("k_fc_chain_bwd<8, 2, 1, false>", "dvae_fc_chain_bwd", "n <= 1024, no conv ends", "fc_chain.hip:786", V + "test_fc_chain_at_the_row_group_switch[1024-10-False]"),
    _v("k_fc_chain_bwd<8, 2, 1, true>", "dvae_fc_chain_bwd", "n <= 1024, convT_gout given", "fc_chain.hip:781", V + "test_fc_chain_at_the_row_group_switch[1024-10-True]"),
    _v("k_fc_chain_bwd<8, 2, 2, false>", "dvae_fc_chain_bwd", "n > 1024, no conv ends", "fc_chain.hip:786", V + "test_fc_chain_at_the_row_group_switch[1025-10-False]"),
    _v("k_fc_chain_bwd<8, 2, 2, true>", "dvae_fc_chain_bwd", "n > 1024, convT_gout given", "fc_chain.hip:781", V + "test_fc_chain_at_the_row_group_switch[1025-10-True]"),
    _v("k_fc_chain_fwd<8, 2, 1, false>", "dvae_fc_chain_fwd", "n_enc <= 1024, no conv ends", "fc_chain.hip:766", V + "test_fc_chain_at_the_row_group_switch[1024-10-False]"),
    _v("k_fc_chain_fwd<8, 2, 1, true>", "dvae_fc_chain_fwd", "n_enc <= 1024, conv_in given", "fc_chain.hip:761", V + "test_fc_chain_at_the_row_group_switch[1024-10-True]"),
    _v("k_fc_chain_fwd<8, 2, 2, false>", "dvae_fc_chain_fwd", "n_enc > 1024, no conv ends", "fc_chain.hip:766", V + "test_fc_chain_at_the_row_group_switch[1025-10-False]"),
    _v("k_fc_chain_fwd<8, 2, 2, true>", "dvae_fc_chain_fwd", "n_enc > 1024, conv_in given", "fc_chain.hip:761", V + "test_fc_chain_at_the_row_group_switch[1025-10-True]"),
]


def _s(launcher, variable, threshold, where, below=None, below_test=None, above=None, above_test=None, reason=None):
    return Switch(launcher, variable, threshold, where, below, below_test, above, above_test, reason)


_BTC = V + "test_btcvae_bwd_at_the_row_switch"
_THIN = V + "test_thin_ends_at_the_wave_specialised_switch"
_KC = V + "test_linear_at_the_contraction_length_switches"
_DISC = V + "test_discriminator_linear_at_the_tile_switches"
_TILES = V + "test_linear_at_the_output_tile_count_switch"
_GRID = V + "test_conv32_at_the_persistent_grid_switch"
_CAP = V + "test_conv_wgrad32_at_the_grid_cap"
_RED = V + "test_wgrad32_at_the_reduction_form_switch"
_CHAIN = V + "test_fc_chain_at_the_row_group_switch"
_SMALL = V + "test_linear_forward_at_the_small_kernel_limits"
_SPLIT = V + "test_linear_at_the_contraction_slice_switches"
_RGRID = V + "test_linear_split_contraction_at_the_reduction_grid_cap"
_DMAMIN = V + "test_linear_at_the_dma_kernel_minima"
_ELT = V + "test_elementwise_kernels_at_their_grid_caps"
_PAST = V + "test_thin_ends_past_the_wave_specialised_switch"
_U8F = T + "test_u8_thin_kernels_vs_fp64"
_FUSED = T + "test_fused_convT3_likelihood_at_the_grid_cap"
_STG = T + "test_staged_convT3_at_the_grid_caps"
_WG4 = T + "test_wgrad32_4x4_at_the_grid_cap"
_GEN = T + "test_generic_conv_at_the_grid_cap"
_RR = T + "test_recon_rows_at_the_slice_switches"
_ADAMC = T + "test_adam_at_the_chunk_switch"

SWITCHES = [
    _s("launch_btcvae_bwd", "Bl", "BTC_WG_MAX_ROWS = 512", "loss.hip:768", "Bl = 512, D = 10", _BTC + "[512-10-True]", "Bl = 513, D = 10", _BTC + "[513-10-True]"),
    _s("launch_btcvae_bwd", "Bl (run-time D)", "BTC_WG_MAX_ROWS = 512", "loss.hip:768", "Bl = 512, D = 6", _BTC + "[512-6-True]", "Bl = 513, D = 6", _BTC + "[513-6-True]"),
    _s("launch_btcvae_bwd", "Bl of a row shard (Bl < Bg)", "BTC_WG_MAX_ROWS = 512", "loss.hip:768", "Bg = 1100, rows [0, 500)",
       V + "test_btcvae_bwd_sharded_with_more_than_512_local_rows[0-500]", "Bg = 1100, rows [500, 1100)",
       V + "test_btcvae_bwd_sharded_with_more_than_512_local_rows[500-600]"),
    _s("reparam_kl_blocks", "ceil(B / 256)", "1 | 2 blocks", "loss.hip:799", "B = 256", V + "test_reparam_kl_at_the_partial_block_switches[256]",
       "B = 257", V + "test_reparam_kl_at_the_partial_block_switches[257]"),
    _s("reparam_kl_blocks", "ceil(B / 256)", "RK_BLOCKS = 64", "loss.hip:800", "B = 16384", V + "test_reparam_kl_at_the_partial_block_switches[16384]",
       "B = 16385", V + "test_reparam_kl_at_the_partial_block_switches[16385]"),
    _s("launch_down_thin_ws", "N", "192", "conv_thin_ws.hip:323", "N = 191, C = 1", _THIN + "[191-1]", "N = 192, C = 1", _THIN + "[192-1]"),
    _s("launch_down_thin_ws", "N (3 channels)", "192", "conv_thin_ws.hip:323", "N = 191, C = 3", _THIN + "[191-3]", "N = 192, C = 3", _THIN + "[192-3]"),
    _s("launch_wgrad_thin_ws", "N", "192", "conv_thin_ws.hip:624", "N = 191", _THIN + "[191-3]", "N = 192", _THIN + "[192-3]"),
    _s("launch_wgrad_ws_t", "N (grid cap on)", "128", "conv_wgrad_ws.hip:305", "N = 128, HS 16", _CAP + "[128-16]", "N = 129, HS 16", _CAP + "[129-16]"),
    _s("launch_wgrad_ws_t", "N (grid cap off)", "320", "conv_wgrad_ws.hip:305", "N = 320, HS 16", _CAP + "[320-16]", "N = 321, HS 16", _CAP + "[321-16]"),
    _s("launch_wgrad_ws_t", "N (grid cap on, HS 8)", "128", "conv_wgrad_ws.hip:305", "N = 128, HS 8", _CAP + "[128-8]", "N = 129, HS 8", _CAP + "[129-8]"),
    _s("launch_wgrad_ws_t", "N (grid cap off, HS 8)", "320", "conv_wgrad_ws.hip:305", "N = 320, HS 8", _CAP + "[320-8]", "N = 321, HS 8", _CAP + "[321-8]"),
    _s("launch_wgrad32_reduce", "N", "WGR_LEAN_MIN_IMAGES = 768", "conv_mfma.hip:372", "N = 767, HS 8", _RED + "[767-8-False-False]", "N = 768, HS 8", _RED + "[768-8-False-False]"),
    _s("launch_wgrad32_reduce", "N (behind k_wgrad32<4>, NHWC)", "768", "conv_mfma.hip:372", "N = 767, HS 4", _RED + "[767-4-False-False]", "N = 768, HS 4", _RED + "[768-4-False-False]"),
    _s("launch_wgrad32_reduce", "N (behind k_wgrad32<4>, NCHW small side)", "768", "conv_mfma.hip:372", "N = 767, HS 4", _RED + "[767-4-True-True]", "N = 768, HS 4", _RED + "[768-4-True-True]"),
    _s("launch_down_dma_t / launch_up_ws_t", "units = N * Hs * Hs / 64", "256 (HS 16)", "conv_down_dma.hip:222", "N = 64", _GRID + "[64-16]", "N = 65", _GRID + "[65-16]"),
    _s("launch_down_dma_t / launch_up_ws_t", "units", "256 (HS 8)", "conv_up_ws.hip:348", "N = 256", _GRID + "[256-8]", "N = 257", _GRID + "[257-8]"),
    _s("launch_down_t<4> / launch_up_t<4>", "units = ceil(N / 4)", "256", "conv_mfma.hip:387", "N = 1024", _GRID + "[1024-4]", "N = 1025", _GRID + "[1025-4]"),
    _s("launch_wgrad_generic", "chunks = N * Hs * Ws / 1024", "2", "conv_generic.hip:385", "N = 7 (16x16)", V + "test_generic_wgrad_at_the_chunk_switches[7]",
       "N = 8", V + "test_generic_wgrad_at_the_chunk_switches[8]"),
    _s("launch_wgrad_generic", "chunks", "64", "conv_generic.hip:384", "N = 256 (64 chunks)", V + "test_generic_wgrad_at_the_chunk_switches[256]",
       "N = 260 (65 -> 64)", V + "test_generic_wgrad_at_the_chunk_switches[260]"),
    _s("fc_chain_rows", "n", "FCC_R4_MAX_ROWS = 1024", "fc_chain.hip:746", "n = 1024", _CHAIN + "[1024-10-False]", "n = 1025", _CHAIN + "[1025-10-False]"),
    _s("fc_chain_rows", "n (with the conv ends)", "1024", "fc_chain.hip:746", "n = 1024", _CHAIN + "[1024-10-True]", "n = 1025", _CHAIN + "[1025-10-True]"),
    _s("fc_chain_rows", "n (run-time D)", "1024", "fc_chain.hip:746", "n = 1024, D = 6", _CHAIN + "[1024-6-True]", "n = 1025, D = 6", _CHAIN + "[1025-6-True]"),
    _s("try_fc32", "Kc", "32", "linear.hip:427", "K = N = 32", _KC + "[32]", "K = N = 36", _KC + "[36]"),
    _s("try_fc32", "Kc", "64", "linear.hip:428", "K = N = 64", _KC + "[64]", "K = N = 68", _KC + "[68]"),
    _s("try_fc32", "Kc", "128", "linear.hip:429", "K = N = 128", _KC + "[128]", "K = N = 132", _KC + "[132]"),
    _s("try_fc32", "Kc", "256", "linear.hip:430", "K = N = 256", _KC + "[256]", "K = N = 260", _KC + "[260]"),
    _s("try_fc32", "Kc", "512", "linear.hip:412", "K = N = 512", _KC + "[512]", "K = N = 516", _KC + "[516]"),
    _s("try_fc32", "output tiles (forward)", "512", "linear.hip:413", "2048 x 960", _TILES + "[2048-64-960-parts0]", "2048 x 1024", _TILES + "[2048-64-1024-parts1]"),
    _s("try_fc32", "output tiles (input gradient)", "512", "linear.hip:413", "2048 x 960", _TILES + "[2048-960-64-parts2]", "2048 x 1024", _TILES + "[2048-1024-64-parts3]"),
    _s("try_fcw32", "output tiles", "512", "linear.hip:536", "960 x 2048", _TILES + "[40-2048-960-parts4]", "1024 x 2048", _TILES + "[40-2048-1024-parts5]"),
    _s("try_fcw32", "M", "64", "linear.hip:538", "M = 64", V + "test_linear_wgrad_at_the_batch_switches[64]", "M = 65", V + "test_linear_wgrad_at_the_batch_switches[65]"),
    _s("try_fcw32", "M", "4096", "linear.hip:534", "M = 4096", V + "test_linear_wgrad_at_the_batch_switches[4096]", "M = 4100", V + "test_linear_wgrad_at_the_batch_switches[4100]"),
    _s("try_gdma_wgrad", "M", "64", "gemm_dma.hip:517", "M = 63", _DISC + "[63]", "M = 64", _DISC + "[64]"),
    _s("try_gdma", "ceil(M / 64) * cols64", "192", "gemm_dma.hip:489", "M = 704", _DISC + "[704]", "M = 705", _DISC + "[705]"),
    _s("try_gdma", "ceil(M / 128) * cols64", "224", "gemm_dma.hip:489", "M = 1664", _DISC + "[1664]", "M = 1665", _DISC + "[1665]"),
    _s("try_narrow_fwd / try_narrow_dgrad", "K", "256", "linear_narrow.hip:88", "K = 252", V + "test_narrow_output_linear_at_its_minimum_contraction[252]",
       "K = 256", V + "test_narrow_output_linear_at_its_minimum_contraction[256]"),
    _s("try_narrow_fwd / try_narrow_dgrad", "N", "NARROW_MAX = 8", "linear_narrow.hip:88", "N = 8", V + "test_linear_outside_the_lds_resident_kernels[100-256-8]",
       "N = 9", V + "test_linear_outside_the_lds_resident_kernels[100-256-9]"),
    _s("launch_linear_wgrad_grouped", "max M", "64", "linear_grouped.hip:165", "M = 64", K + "test_linear_wgrad_grouped[64]", "M = 65", V + "test_linear_wgrad_grouped_past_its_slab_switches[65]"),
    _s("launch_linear_wgrad_grouped", "max M", "128", "linear_grouped.hip:166", "M = 128", K + "test_linear_wgrad_grouped[128]", "M = 129", V + "test_linear_wgrad_grouped_past_its_slab_switches[129]"),
    _s("launch_adam", "nt", "ADAM_MAX_T = 64", "adam.hip:80", "64 tensors", V + "test_adam_at_the_table_split[64]", "65 tensors", V + "test_adam_at_the_table_split[65]"),
    # ---- linear.hip behind try_fc32 / try_gdma
    _s("use_small", "Kc", "4096", "linear.hip:567", "K = 4096", _SMALL + "[40-4096-36]", "K = 4100", _SMALL + "[40-4100-36]"),
    _s("use_small", "tiles64", "192", "linear.hip:567", "6080 x 100 (190 tiles)", _SMALL + "[6080-516-100]", "6081 x 100 (192)", _SMALL + "[6081-516-100]"),
    _s("pick_split", "Kc / (2 S) (S = 1 | 2)", "64", "linear.hip:615", "K = 127", _SPLIT + "[40-127-36-parts0]", "K = 129", _SPLIT + "[40-129-36-parts1]"),
    _s("pick_split", "Kc / (2 S) (S = 8 | 16)", "64", "linear.hip:615", "K = 1023", _SPLIT + "[40-1023-36-parts2]", "K = 1025", _SPLIT + "[40-1025-36-parts3]"),
    _s("pick_split", "S", "16", "linear.hip:615", "K = 1025 (S = 16 wanted)", _SPLIT + "[40-1025-36-parts3]", "K = 2049 (32 wanted)", _SPLIT + "[40-2049-36-parts4]"),
    _s("pick_split", "tiles * S", "256", "linear.hip:615", "1024 x 960 (240 tiles)", _SPLIT + "[1024-129-960-parts5]", "1024 x 1024 (256)", _SPLIT + "[1024-129-1024-parts6]"),
    _s("launch_linear_wgrad", "M / (2 S)", "64", "linear.hip:717", "M = 127", _SPLIT + "[127-513-512-parts7]", "M = 129", _SPLIT + "[129-513-512-parts8]"),
    _s("launch_linear_fwd", "k_splitk_epilogue grid", "1024", "linear.hip:653", "512 x 512", _RGRID + "[512-301-512-parts0]", "512 x 516", _RGRID + "[512-301-516-parts1]"),
    _s("launch_linear_dgrad", "k_splitk_epilogue grid", "1024", "linear.hip:692", "512 x 512", _RGRID + "[512-512-301-parts2]", "512 x 516", _RGRID + "[512-516-301-parts3]"),
    _s("launch_linear_wgrad", "k_splitk_reduce grid", "1024", "linear.hip:733", "512 x 511", _RGRID + "[300-511-512-parts4]", "512 x 513", _RGRID + "[300-513-512-parts5]"),
    _s("try_gdma", "Kc", "256", "gemm_dma.hip:482", "K = 252", _DMAMIN + "[2048-252-1024-parts0]", "K = 256", _DMAMIN + "[2048-256-1024-parts1]"),
    _s("try_gdma", "N (forward)", "128", "gemm_dma.hip:482", "N = 124", _DMAMIN + "[40-516-124-parts2]", "N = 128", _DMAMIN + "[40-516-128-parts3]"),
    _s("try_gdma", "N (input gradient: the K columns)", "128", "gemm_dma.hip:482", "K = 124", _DMAMIN + "[40-124-516-parts4]", "K = 128", _DMAMIN + "[40-128-516-parts5]"),
    _s("try_gdma_wgrad", "output tiles", "128", "gemm_dma.hip:518", "512 x 960 (120)", _DMAMIN + "[100-960-512-parts6]", "512 x 1024 (128)", _DMAMIN + "[100-1024-512-parts7]"),
    _s("try_narrow_dgrad", "blocks", "4096", "linear_narrow.hip:101", "M = 16384", V + "test_narrow_input_gradient_at_its_grid_cap[16384]",
       "M = 16388", V + "test_narrow_input_gradient_at_its_grid_cap[16388]"),
    # ---- loss.hip, loglik.hip
    _s("launch_sigmoid_bwd", "workgroups", "4096", "loss.hip:825", "n = 2^20", _ELT + "[0]", "n = 2^20 + 1", _ELT + "[1]"),
    _s("launch_u8_to_f32", "workgroups", "4096", "loss.hip:845", "n = 2^24", _ELT + "[0]", "n = 2^24 + 16", _ELT + "[1]"),
    _s("launch_add", "workgroups", "2048", "loss.hip:860", "n = 2^19", _ELT + "[0]", "n = 2^19 + 1", _ELT + "[1]"),
    _s("launch_axpby", "workgroups", "2048", "loss.hip:867", "n = 2^19", _ELT + "[0]", "n = 2^19 + 1", _ELT + "[1]"),
    _s("launch_recon_rows", "nslice = ceil(row_elems / 4 / 256)", "1 | 2 (k_recon_rows_finish)", "loglik.hip:147", "1024 elements, K = 1",
       _RR + "[bernoulli-False-1024-1]", "1028 elements, K = 1", _RR + "[bernoulli-False-1028-1]"),
    _s("launch_recon_rows", "nslice (two row chunks, uint8 target)", "2 | 3", "loglik.hip:147", "2048 elements, K = 9", _RR + "[laplace-True-2048-9]",
       "2052 elements, K = 9", _RR + "[laplace-True-2052-9]"),
    # ---- persistent-grid caps: the image count from which a workgroup takes a second trip (more trip counts: TRIP_CLASSES)
    _s("launch_down_thin", "n_units = 8 N", "1536", "conv_thin.hip:679", "N = 192, C = 1 (k_down_thin<1, 1>)", _THIN + "[192-1]",
       "N = 193, C = 1", _PAST + "[193-1]"),
    _s("launch_down_thin", "n_units = 8 N (3 channels)", "1536", "conv_thin.hip:679", "N = 192, C = 3 (k_down_thin<3, 1>)", _THIN + "[192-3]",
       "N = 193, C = 3 (and modes 0, 2, 3 on unaligned buffers)", V + "test_thin_ends_past_the_cap_on_buffers_the_wave_specialised_kernels_decline"),
    _s("launch_down_thin_u8", "n_units = 8 N", "1536", "conv_thin.hip:719", "N = 192", _U8F + "[192-1-0]", "N = 193", _U8F + "[193-1-1]"),
    _s("launch_up_thin_recon", "n_units = 8 N", "1536", "conv_thin.hip:708", "N = 192, C = 1", _FUSED + "[192-1-0-False]", "N = 193, C = 1", _FUSED + "[193-1-1-False]"),
    _s("launch_up_thin_recon", "n_units = 8 N (3 channels)", "1536", "conv_thin.hip:708", "N = 192, C = 3", _FUSED + "[192-3-2-False]", "N = 193, C = 3", _FUSED + "[193-3-0-False]"),
    _s("launch_up_thin_recon_u8", "n_units = 8 N", "1536", "conv_thin.hip:733", "N = 192, C = 1", _FUSED + "[192-1-1-True]", "N = 193, C = 1", _FUSED + "[193-1-2-True]"),
    _s("launch_up_thin_recon_u8", "n_units = 8 N (3 channels)", "1536", "conv_thin.hip:733", "N = 192, C = 3", _FUSED + "[192-3-0-True]", "N = 193, C = 3", _FUSED + "[193-3-1-True]"),
    _s("k_up_thin / k_up_thin_pk", "XCD-aware unit map: grid % 64", "0", "conv_thin.hip:214", "N = 8 (64 workgroups: on)", _FUSED + "[8-3-2-False]",
       "N = 9 (72: off)", _FUSED + "[9-3-2-False]"),
    _s("launch_up_thin_staged", "n_units = 8 N (k_up_thin_pk<1, *>)", "1536", "conv_thin.hip:545", "N = 192", _STG + "[192-1]", "N = 193", _STG + "[193-1]"),
    _s("launch_up_thin_staged", "n_units = 8 N (k_up_thin_pk<3, *>: buffers k_up_thin_mm declines)", "1536", "conv_thin.hip:545", "N = 3 (24 units)",
       V + "test_convT3_staged_falls_back_to_the_packed_fma_kernel", "N = 193", V + "test_convT3_staged_fallback_past_its_grid_cap"),
    _s("launch_up_thin_mm", "n_units = 3 N", "512", "conv_up_thin_mm.hip:278", "N = 170 (510 units)", _STG + "[170-3]", "N = 171 (513)", _STG + "[171-3]"),
    _s("launch_wgrad_thin_u8", "n_units = 8 N", "WT_MAX_BLOCKS = 512", "conv_thin.hip:757", "N = 64, C = 3", _U8F + "[64-3-0]", "N = 65, C = 1", _U8F + "[65-1-1]"),
    _s("launch_wgrad_thin_u8", "n_units = 8 N (uint8 == fp32 kernel, bit for bit)", "512", "conv_thin.hip:757", "N = 64, C = 3",
       U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[64-3]", "N = 65, C = 3", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[65-3]"),
    _s("launch_wgrad_thin", "n_units = 8 N (fp32; aligned buffers leave for conv_thin_ws.hip at 192 images)", "512", "conv_thin.hip:772",
       "N = 64, C = 3", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[64-3]", "N = 65, C = 1", U8 + "test_u8_kernels_equal_fp32_kernels_bitwise[65-1]"),
    _s("launch_wgrad_t<4> (k_wgrad32<4>)", "units = ceil(N / 4)", "WG_MAX_BLOCKS = 256", "conv_mfma.hip:425", "N = 1024", _WG4 + "[1024-False-False]",
       "N = 1025", _WG4 + "[1025-False-False]"),
    _s("launch_wgrad_t<4> (k_wgrad32<4>)", "units (convT, NCHW small side)", "256", "conv_mfma.hip:425", "N = 1024", _WG4 + "[1024-True-True]",
       "N = 1025", _WG4 + "[1025-True-True]"),
    _s("grid_for (k_down_thin_px<1>)", "ceil(N * Hs * Ws * 8 / 256)", "8192", "conv_generic.hip:344", "N = 16384 (8x8 images)", _GEN + "[down_thin_px1-0]",
       "N = 16385 (8193 wanted)", _GEN + "[down_thin_px1-1]"),
    _s("grid_for (k_down_thin_px<3>)", "ceil(N * Hs * Ws * 8 / 256)", "8192", "conv_generic.hip:344", "N = 16384 (8x8 images)", _GEN + "[down_thin_px3-0]",
       "N = 16385", _GEN + "[down_thin_px3-1]"),
    _s("grid_for (k_down_generic)", "ceil(N * Cs * Hs * Ws / 256)", "8192", "conv_generic.hip:351", "N = 8192 (2 -> 16 channels, 8x8 -> 4x4)",
       _GEN + "[down_generic-0]", "N = 8193", _GEN + "[down_generic-1]"),
    _s("grid_for (k_up_thin_px<1>)", "ceil(N * Cb * 4 Hs Ws / 256)", "8192", "conv_generic.hip:363", "N = 8192 (8x8 -> 16x16)", _GEN + "[up_thin_px1-0]",
       "N = 8193", _GEN + "[up_thin_px1-1]"),
    _s("grid_for (k_up_thin_px<3>)", "ceil(N * Cb * 4 Hs Ws / 256)", "8192", "conv_generic.hip:363", "N = 10922 (4x4 -> 8x8: 8191.5)", _GEN + "[up_thin_px3-0]",
       "N = 10923 (8192.25)", _GEN + "[up_thin_px3-1]"),
    _s("grid_for (k_up_generic)", "ceil(N * Cb * 4 Hs Ws / 256)", "8192", "conv_generic.hip:370", "N = 8192 (2 -> 4 channels, 4x4 -> 8x8)",
       _GEN + "[up_generic-0]", "N = 8193", _GEN + "[up_generic-1]"),
    _s("launch_wgrad_generic", "chunks * Cs * Cb * 17 floats against the workspace", "dvae_conv_wgrad_ws_floats() = 4 276 224", "conv_generic.hip:385",
       "N = 61 (64 -> 64 channels, 32x32 small side)", T + "test_generic_wgrad_at_the_workspace_switch[61]", "N = 62",
       T + "test_generic_wgrad_at_the_workspace_switch[62]"),
    _s("k_adam", "tensor elements", "ADAM_CHUNK = 4096 (and 8192: 2 | 3 workgroups)", "adam.hip:88", "4096 and 8192 elements", _ADAMC + "[0]",
       "4097 and 8193 elements", _ADAMC + "[1]"),
    # ---- read in a launcher, out of reach of the C-ABI
    _s("pick_split / launch_linear_wgrad", "S * (output + 4096) floats against the workspace", "dvae_conv_wgrad_ws_floats()", "linear.hip:616",
       reason="the loop in front of the clamp doubles S only while tiles * S < 256 and S < 16, so tiles * S < 512 and S <= 16 behind it, and "
              "the output has at most 4096 tiles elements (tiles = ceil(rows / 64) * ceil(columns / 64), linear.hip:640 / 679): S * (output + "
              "4096) <= 4096 (tiles * S + S) < 4096 * 528 = PICK_SPLIT_WS_BOUND floats; launch_linear_wgrad's own form (linear.hip:718) needs "
              "S * (N * K + N) <= 4096 tiles * S + 64 tiles * S < 4160 * 512, which is less.  capi.hip passes dvae_conv_wgrad_ws_floats() = "
              "4 276 224 floats on every call, so neither clamp ever halves S; test_kernel_variants_host.py::"
              "test_the_workspace_keeps_the_split_contraction_clamps_out_of_reach fails if the workspace shrinks below the bound"),
]

# above every S * (out_elems + 4096) that pick_split's clamp (linear.hip:616) can meet: tiles * S < 512 and S <= 16 behind its first loop
PICK_SPLIT_WS_BOUND = 4096 * 512 + 4096 * 16

# Thresholds read in the launchers that have no entry above: none.  A newly found one goes into SWITCHES with its pair.
OPEN_SWITCHES = []


def _t(family, where, grid, trips, depth, n_from, cases, unreachable=None):
    return TripFamily(family, where, grid, trips, depth, n_from, cases, unreachable or {})


_STRIDE = "cdiv(units - b, grid)"                                    # for (unit = b; unit < units; unit += grid)
_XMAP = "cdiv(8 * N - (8 * ((b & 7) + 8 * (b >> 6)) + ((b >> 3) & 7) if grid % 64 == 0 else b), grid)"     # conv_thin.hip:214-217
_LANE = "cdiv(N - ((b & 7) + 8 * (b >> 6)), grid >> 3)"              # conv_thin_ws.hip:65-68, 113: n0 .. N step grid / 8 images
_W4T = T + "test_wgrad32_4x4_trip_counts"
_WWS = T + "test_wgrad32ws_trip_counts"

# cases: (class, N, test id): "u<t>" = t trips in every workgroup, "m<t>" = workgroups of t + 1 and of t trips.  In the expressions
# N is the image count, b the workgroup, grid the grid size, units the `units` expression, cdiv(a, b) = max(0, ceil(a / b)).
TRIP_CLASSES = [
    _t("k_down_thin_ws", "conv_thin_ws.hip:324", "512", _LANE, depth=4, n_from=192, cases=[       # ring of four tile stages
        ("u3", 192, _THIN + "[192-3]"), ("u4", 256, _PAST + "[256-1]"), ("u5", 320, _PAST + "[320-3]"),
        ("u16", 1024, B + "test_conv_persistent_loops[1024-3-64]"), ("m3", 193, _PAST + "[193-1]"), ("m3", 224, _PAST + "[224-3]"),
        ("m4", 257, _PAST + "[257-3]")]),
    _t("k_wgrad_thin_ws", "conv_thin_ws.hip:631", "256", _LANE, depth=3, n_from=192, cases=[      # ring of three
        ("u6", 192, _THIN + "[192-1]"), ("u7", 224, _PAST + "[224-3]"), ("u8", 256, _PAST + "[256-1]"), ("u10", 320, _PAST + "[320-3]"),
        ("m6", 193, _PAST + "[193-3]"), ("m8", 257, _PAST + "[257-1]")]),
    _t("k_down_thin", "conv_thin.hip:679", "min(8 * N, 1536)", _STRIDE.replace("units", "8 * N"), depth=2, n_from=1, cases=[   # two tiles in registers
        ("u1", 191, _THIN + "[191-1]"), ("u2", 384, _U8F + "[384-3-1]"), ("u3", 576, _U8F + "[576-1-0]"), ("u4", 768, _U8F + "[768-1-1]"),
        ("m1", 193, _PAST + "[193-1]")]),
    _t("k_up_thin fused", "conv_thin.hip:708", "min(8 * N, 1536)", _XMAP, depth=1, n_from=1, cases=[
        ("u1", 192, _FUSED + "[192-1-0-False]"), ("u2", 384, _U8F + "[384-3-1]"), ("u3", 576, _U8F + "[576-1-0]"),
        ("m1", 193, _FUSED + "[193-3-0-False]")]),
    _t("k_up_thin_pk", "conv_thin.hip:545", "min(8 * N, 1536)", _XMAP, depth=1, n_from=1, cases=[
        ("u1", 192, _STG + "[192-1]"), ("u2", 384, _STG + "[384-1]"), ("u3", 576, _STG + "[576-1]"), ("m1", 193, _STG + "[193-1]")]),
    _t("k_up_thin_mm", "conv_up_thin_mm.hip:278", "min(3 * N, 512)", _STRIDE.replace("units", "3 * N"), depth=2, n_from=1, cases=[   # next tile in registers
        ("u1", 170, _STG + "[170-3]"), ("u3", 512, _STG + "[512-3]"), ("u6", 1024, _STG + "[1024-3]"), ("m1", 171, _STG + "[171-3]")],
       unreachable={2: "3 N is a multiple of the 512 workgroups only for N = 512 k, which gives 3 k trips"}),
    _t("k_wgrad_thin", "conv_thin.hip:757", "min(8 * N, 512)", _STRIDE.replace("units", "8 * N"), depth=2, n_from=1, cases=[   # next unit in registers
        ("u1", 64, _U8F + "[64-3-0]"), ("u2", 128, _U8F + "[128-3-2]"), ("u3", 192, _U8F + "[192-1-0]"), ("u4", 256, _U8F + "[256-3-0]"),
        ("m1", 65, _U8F + "[65-1-1]")]),
    _t("k_wgrad32<4>", "conv_mfma.hip:425", "min(cdiv(N, 4), 256)", _STRIDE.replace("units", "cdiv(N, 4)"), depth=2, n_from=1, cases=[
        ("u1", 1024, _WG4 + "[1024-False-False]"), ("u2", 2048, _W4T + "[2048]"), ("u3", 3072, _W4T + "[3072]"), ("u4", 4096, _W4T + "[4096]"),
        ("m1", 1025, _WG4 + "[1025-False-False]")]),
    _t("k_down32dma / k_up32ws (HS 16)", "conv_down_dma.hip:222", "min(4 * N, 256)", _STRIDE.replace("units", "4 * N"), depth=3, n_from=1, cases=[
        ("u1", 64, _GRID + "[64-16]"), ("u2", 128, _GRID + "[128-16]"), ("u3", 192, _GRID + "[192-16]"), ("u4", 256, _GRID + "[256-16]"),
        ("u5", 320, _GRID + "[320-16]"), ("m1", 65, _GRID + "[65-16]"), ("m2", 129, _GRID + "[129-16]"), ("m3", 193, _GRID + "[193-16]")]),
    _t("k_wgrad32ws (HS 16)", "conv_wgrad_ws.hip:307", "min(4 * N, 192 if 128 < N <= 320 else 256)", _STRIDE.replace("units", "4 * N"), depth=4,
       n_from=1, cases=[                                             # two LDS buffers and two register sets
        ("u1", 64, _WWS + "[64]"), ("u2", 128, _CAP + "[128-16]"), ("u3", 144, _WWS + "[144]"), ("u4", 192, _WWS + "[192]"),
        ("u5", 240, _WWS + "[240]"), ("u6", 288, _WWS + "[288]"), ("m2", 129, _CAP + "[129-16]")]),
]



# ---- PREDICATES: the non-numeric terms of the conv / linear launcher conditions ------------------------------------------------
# A conv case is the geometry both directions of the k4/s2/p1 family run at: big[N,Cb,H,W] <-> small[N,Cs,H/2,W/2], the layouts
# of the two sides and the forward activation; `null` names a pointer role passed as NULL (b, db, mask, ws), `off` a role and a
# byte offset into a larger 16-byte-aligned buffer (roles: big, small, w, b, mask, dw, db, ws).  A linear case is (M, K, N), the
# forward activation and `off` (roles: x, w, b, y, dy, x_act, dx, dw, db).  tests/test_gpu_dispatch_predicates.py runs every
# entry point of the family at each case; the id functions below spell the pytest ids.
CONV_BASE = dict(N=3, Cb=32, Cs=32, H=32, W=32, bl="NHWC", sl="NHWC", act="relu", null=None, off=None)
THIN_BASE = dict(N=3, Cb=3, Cs=32, H=64, W=64, bl="NCHW", sl="NHWC", act="relu", null=None, off=None)
LIN_BASE = dict(M=8, K=512, N=256, act="relu", off=None)


def conv_case(_base=None, **kw):
    d = dict(_base or CONV_BASE)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


def thin_case(**kw):
    return conv_case(THIN_BASE, **kw)


def lin_case(**kw):
    d = dict(LIN_BASE)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


def conv_id(d):
    s = "N%d-Cb%d-Cs%d-%dx%d-b%s-s%s-%s" % (d["N"], d["Cb"], d["Cs"], d["H"], d["W"], d["bl"], d["sl"], d["act"])
    if d["null"]:
        s += "-null_" + d["null"]
    if d["off"]:
        s += "-%s_plus%d" % d["off"]
    return s


def lin_id(d):
    s = "M%d-K%d-N%d-%s" % (d["M"], d["K"], d["N"], d["act"])
    if d["off"]:
        s += "-%s_plus%d" % d["off"]
    return s


Predicate = namedtuple("Predicate", "launcher term where family entry base arg neighbour kernel base_test test reason")

P = "tests/test_gpu_dispatch_predicates.py::"
_FAMILY_TEST = {"conv": ("test_conv_family", conv_id), "fused": ("test_fused_likelihood", conv_id), "linear": ("test_linear_family", lin_id)}


def _p(launcher, where, term, family, entry, base, arg, value, kernel, base_test=None, test=None):
    """One term of a launcher condition: `base` satisfies the whole conjunction the term stands in, the neighbour is `base`
    with the argument(s) `arg` set to `value` -- the term negated alone -- and `kernel` is what then takes the call of `entry`
    (read from the launchers, as VARIANTS is).  arg "H,W" is the one argument `image size` of a square image."""
    keys = arg.split(",")
    neighbour = dict(base, **dict(zip(keys, value if len(keys) > 1 else (value,))))
    if family in _FAMILY_TEST:
        fn, ident = _FAMILY_TEST[family]
        base_test, test = P + "%s[%s]" % (fn, ident(base)), P + "%s[%s]" % (fn, ident(neighbour))
    return Predicate(launcher, term, where, family, entry, base, arg, neighbour, kernel, base_test, test, None)


def _unreachable(launcher, where, term, reason):
    return Predicate(launcher, term, where, None, None, None, None, None, None, None, None, reason)


_C, _T, _T1 = conv_case(), thin_case(), thin_case(Cb=1)
_C16, _C8 = conv_case(H=16, W=16), conv_case(H=8, W=8)               # Hs = 8, Hs = 4
_C4N = conv_case(H=8, W=8, sl="NCHW")                                # the 4x4 end with its NCHW small side
_CSIG, _TSIG = conv_case(act="sigmoid"), thin_case(act="sigmoid")    # declined for the activation alone
_PX, _PX1 = thin_case(H=32, W=32), thin_case(Cb=1, H=32, W=32)       # the thin ends at the 32x32 image: k_*_thin_px
_DN, _UP, _WG = "dvae_conv4s2_fwd, dvae_convT4s2_dgrad", "dvae_convT4s2_fwd, dvae_conv4s2_dgrad", "dvae_conv4s2_wgrad, dvae_convT4s2_wgrad"
_GD, _GU, _GW = "k_down_generic", "k_up_generic", "k_wgrad_generic + k_chansum"
_L, _LD, _LN, _LS = lin_case(), lin_case(M=64, K=1000, N=1000), lin_case(M=100, K=1000, N=2), lin_case(K=1000, N=36)
_L12 = lin_case(K=12)
_FW, _DG, _WGL = "dvae_linear_fwd", "dvae_linear_dgrad", "dvae_linear_wgrad"
_GRP = dict(K=512, N=256, x_off=0, dy_off=0)
_GRP_BASE, _GRP_TEST = K + "test_linear_wgrad_grouped[64]", P + "test_linear_wgrad_grouped_flag_bits[8]"
_REFUSED = P + "test_fused_likelihood_refuses_an_unaligned_target_recon_or_gradient[4-target]"
_CALLER = "%s tests the same term before the call (no other caller in the shipped library), so it is always true here"

PREDICATES = [
    # ---- capi.hip: run_down, run_up, run_wgrad, dvae_convT4s2_sigmoid_recon_fwd
    _p("run_down", "capi.hip:31", "aligned16(a.big, a.w, a.bias, a.mask, a.out)", "conv", _DN, _C, "off", ("big", 4), _GD),
    _p("run_up", "capi.hip:42", "aligned16(a.small, a.w, a.bias, a.mask, a.out)", "conv", _UP, _C, "off", ("small", 4), _GU),
    _p("run_wgrad", "capi.hip:57", "ws != nullptr", "conv", _WG, _C, "null", "ws", _GW),
    _p("run_wgrad", "capi.hip:58", "aligned16(big, small, dw, db, ws)", "conv", _WG, _C, "off", ("dw", 4), _GW),
    _p("run_wgrad (4x4 end, NCHW)", "capi.hip:60", "Hs == Ws", "conv", _WG, _C4N, "W", 4, _GW),
    _p("run_wgrad (4x4 end, NCHW)", "capi.hip:60", "Cs == 32", "conv", _WG, _C4N, "Cs", 16, _GW),
    _p("run_wgrad (4x4 end, NCHW)", "capi.hip:60", "Cb == 32", "conv", _WG, _C4N, "Cb", 16, _GW),
    _p("run_wgrad (4x4 end, NCHW)", "capi.hip:60", "big_layout == DVAE_NHWC", "conv", _WG, _C4N, "bl", "NCHW", _GW),
    _p("run_wgrad (4x4 end, NCHW)", "capi.hip:60", "Hs == 4", "conv", _WG, _C4N, "H,W", (16, 16), _GW),
    _p("run_wgrad (4x4 end, NCHW)", "capi.hip:61", "small_layout == DVAE_NCHW", "conv", _WG, _C4N, "sl", "NHWC", "k_wgrad32<4> (capi.hip:64)"),
    _p("run_wgrad", "capi.hip:63", "Hs == Ws", "conv", _WG, _C, "W", 16, _GW),
    _p("run_wgrad", "capi.hip:63", "Cs == 32", "conv", _WG, _C, "Cs", 16, _GW),
    _p("run_wgrad", "capi.hip:63", "small_layout == DVAE_NHWC", "conv", _WG, _C, "sl", "NCHW", _GW),
    _p("run_wgrad", "capi.hip:64", "Cb == 32", "conv", _WG, _C, "Cb", 16, _GW),
    _p("run_wgrad", "capi.hip:64", "big_layout == DVAE_NHWC", "conv", _WG, _C, "bl", "NCHW", _GW),
    _p("run_wgrad", "capi.hip:64", "Hs == 4", "conv", _WG, _C8, "H,W", (4, 4), _GW),
    _p("run_wgrad", "capi.hip:64", "Hs == 8", "conv", _WG, _C16, "H,W", (12, 12), _GW),
    _p("run_wgrad", "capi.hip:64", "Hs == 16", "conv", _WG, _C, "H,W", (64, 64), "k_wgrad_generic_part + k_wgrad_generic_fin"),
    _p("run_wgrad (thin)", "capi.hip:67", "Cb == 1", "conv", _WG, _T1, "Cb", 2, "k_wgrad_generic_part + k_wgrad_generic_fin"),
    _p("run_wgrad (thin)", "capi.hip:67", "Cb == 3", "conv", _WG, _T, "Cb", 4, "k_wgrad_generic_part + k_wgrad_generic_fin"),
    _p("run_wgrad (thin)", "capi.hip:67", "Hs == 32", "conv", _WG, _T, "H,W", (32, 32), _GW),
    _p("run_wgrad (thin)", "capi.hip:67", "big_layout == DVAE_NCHW", "conv", _WG, _T, "bl", "NHWC", "k_wgrad_generic_part + k_wgrad_generic_fin"),
    _p("run_wgrad (thin)", "capi.hip:67", "aligned16(small, ws)", "conv", _WG, _T, "off", ("small", 4), "k_wgrad_generic_part + k_wgrad_generic_fin"),
    _p("dvae_convT4s2_sigmoid_recon_fwd", "capi.hip:142", "aligned16(target, recon, g)", "refusal", "dvae_convT4s2_sigmoid_recon_fwd",
       dict(target_off=0), "target_off", 4, "none: refused by DVAE_CHECK_ARG", P + "test_fused_likelihood[%s]" % conv_id(_T), _REFUSED),
    _p("dvae_convT4s2_sigmoid_recon_fwd", "capi.hip:145", "aligned16(x, w, b)", "fused", "dvae_convT4s2_sigmoid_recon_fwd", _T, "off",
       ("small", 4), "k_up_generic + k_recon_loss"),
    # ---- conv_mfma.hip: mfma32_applicable (l0, l1 = big, small layouts in launch_down_mfma32; small, big in launch_up_mfma32)
    _p("mfma32_applicable", "conv_mfma.hip:439", "Cb == 32", "conv", _DN + ", " + _UP, _C, "Cb", 16, _GD + " / " + _GU),
    _p("mfma32_applicable", "conv_mfma.hip:439", "Cs == 32", "conv", _DN + ", " + _UP, _C, "Cs", 16, _GD + " / " + _GU),
    _p("mfma32_applicable", "conv_mfma.hip:439", "Hs == Ws", "conv", _DN + ", " + _UP, _C, "H", 16, _GD + " / " + _GU),
    _p("mfma32_applicable", "conv_mfma.hip:439", "Hs == 4", "conv", _DN + ", " + _UP, _C8, "H,W", (4, 4), _GD + " / " + _GU),
    _p("mfma32_applicable", "conv_mfma.hip:439", "Hs == 8", "conv", _DN + ", " + _UP, _C16, "H,W", (12, 12), _GD + " / " + _GU),
    _p("mfma32_applicable", "conv_mfma.hip:439", "Hs == 16", "conv", _DN + ", " + _UP, _C, "H,W", (64, 64), _GD + " / " + _GU),
    _p("mfma32_applicable", "conv_mfma.hip:439", "l0 == DVAE_NHWC", "conv", _DN, _C, "bl", "NCHW", _GD),
    _p("mfma32_applicable", "conv_mfma.hip:440", "l1 == DVAE_NHWC", "conv", _DN, _C, "sl", "NCHW", _GD),
    _unreachable("mfma32_applicable", "conv_mfma.hip:440", "l2 == DVAE_NHWC", "both call sites (conv_mfma.hip:446, 456) pass the literal DVAE_NHWC"),
    _p("launch_down_mfma32", "conv_mfma.hip:445", "a.Hs == 4", "conv", _DN, _C4N, "H,W", (16, 16), _GD),
    _p("launch_down_mfma32", "conv_mfma.hip:445", "a.out_layout == DVAE_NCHW", "conv", _DN, _C4N, "sl", "NHWC", "k_down32<4, *> (still)"),
    _p("launch_down_mfma32", "conv_mfma.hip:447", "a.act != DVAE_ACT_NONE", "conv", "dvae_conv4s2_fwd", _CSIG, "act", "none", "k_down32dma<16, false>"),
    _p("launch_down_mfma32", "conv_mfma.hip:447", "a.act != DVAE_ACT_RELU", "conv", "dvae_conv4s2_fwd", _CSIG, "act", "relu", "k_down32dma<16, false>"),
    _p("launch_down_mfma32", "conv_mfma.hip:449", "a.Hs == 16", "conv", _DN, _C, "H,W", (16, 16), "k_down32dma<8, *> (still)"),
    _p("launch_down_mfma32", "conv_mfma.hip:449", "a.Hs == 8", "conv", _DN, _C16, "H,W", (8, 8), "k_down32<4, *>"),
    _p("launch_up_mfma32", "conv_mfma.hip:455", "a.Hs == 4", "conv", _UP, _C4N, "H,W", (16, 16), _GU),
    _p("launch_up_mfma32", "conv_mfma.hip:455", "a.small_layout == DVAE_NCHW", "conv", _UP, _C4N, "sl", "NHWC", "k_up32<4, *> (still)"),
    _p("launch_up_mfma32", "conv_mfma.hip:457", "a.act != DVAE_ACT_NONE", "conv", "dvae_convT4s2_fwd", conv_case(H=8, W=8, act="sigmoid"), "act", "none", "k_up32<4, false>"),
    _p("launch_up_mfma32", "conv_mfma.hip:457", "a.act != DVAE_ACT_RELU", "conv", "dvae_convT4s2_fwd", conv_case(H=8, W=8, act="sigmoid"), "act", "relu", "k_up32<4, false>"),
    _p("launch_wgrad_mfma32", "conv_mfma.hip:468", "Hs == 16", "conv", _WG, _C, "H,W", (16, 16), "k_wgrad32ws<8> (still)"),
    _p("launch_wgrad_mfma32", "conv_mfma.hip:468", "Hs == 8", "conv", _WG, _C16, "H,W", (8, 8), "k_wgrad32<4>"),
    # ---- conv_up_ws.hip: launch_up_mfma32_ws
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:382", "a.Cb == 32", "conv", _UP, _C, "Cb", 16, _GU),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:382", "a.Cs == 32", "conv", _UP, _C, "Cs", 16, _GU),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:382", "a.Hs == a.Ws", "conv", _UP, _C, "W", 16, _GU),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:382", "a.Hs == 8", "conv", _UP, _C16, "H,W", (8, 8), "k_up32<4, *> (launch_up_mfma32)"),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:382", "a.Hs == 16", "conv", _UP, _C, "H,W", (64, 64), _GU),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:382", "a.small_layout == DVAE_NHWC", "conv", _UP, _C, "sl", "NCHW", _GU),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:383", "a.out_layout == DVAE_NHWC", "conv", _UP, _C, "bl", "NCHW", _GU),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:385", "a.act != DVAE_ACT_NONE", "conv", "dvae_convT4s2_fwd", _CSIG, "act", "none", "k_up32ws<16, 0, false>"),
    _p("launch_up_mfma32_ws", "conv_up_ws.hip:385", "a.act != DVAE_ACT_RELU", "conv", "dvae_convT4s2_fwd", _CSIG, "act", "relu", "k_up32ws<16, 0, false>"),
    # ---- conv_thin.hip: thin_applicable and the layout / activation / alignment terms beside it
    _p("thin_applicable", "conv_thin.hip:671", "a.Cb == 1", "conv", _DN + ", " + _UP, _T1, "Cb", 2, _GD + " / " + _GU),
    _p("thin_applicable", "conv_thin.hip:671", "a.Cb == 3", "conv", _DN + ", " + _UP, _T, "Cb", 4, _GD + " / " + _GU),
    _p("thin_applicable", "conv_thin.hip:671", "a.Cs == 32", "conv", _DN + ", " + _UP, _T, "Cs", 16, _GD + " / " + _GU),
    _p("thin_applicable", "conv_thin.hip:671", "a.Hs == 32", "conv", _DN + ", " + _UP, _T, "H", 32, "k_down_thin_px<3> / k_up_thin_px<3>"),
    _p("thin_applicable", "conv_thin.hip:671", "a.Ws == 32", "conv", _DN + ", " + _UP, _T, "W", 32, "k_down_thin_px<3> / k_up_thin_px<3>"),
    _p("launch_down_thin", "conv_thin.hip:675", "a.big_layout != DVAE_NCHW", "conv", _DN, _T, "bl", "NHWC", _GD),
    _p("launch_down_thin", "conv_thin.hip:675", "a.out_layout != DVAE_NHWC", "conv", _DN, _T, "sl", "NCHW", _GD),
    _p("launch_down_thin", "conv_thin.hip:676", "a.act != DVAE_ACT_NONE", "conv", "dvae_conv4s2_fwd", _TSIG, "act", "none", "k_down_thin<3, 0, float>"),
    _p("launch_down_thin", "conv_thin.hip:676", "a.act != DVAE_ACT_RELU", "conv", "dvae_conv4s2_fwd", _TSIG, "act", "relu", "k_down_thin<3, 0, float>"),
    _p("launch_up_thin", "conv_thin.hip:694", "a.small_layout != DVAE_NHWC", "conv", "dvae_convT4s2_fwd", _T, "sl", "NCHW", _GU),
    _p("launch_up_thin", "conv_thin.hip:694", "a.out_layout != DVAE_NCHW", "conv", "dvae_convT4s2_fwd", _T, "bl", "NHWC", "k_up_thin_px<3>"),
    _p("launch_up_thin", "conv_thin.hip:694", "a.act == DVAE_ACT_LEAKY02", "conv", "dvae_convT4s2_fwd", _T, "act", "leaky", "k_up_thin_px<3>"),
    _p("launch_up_thin", "conv_thin.hip:695", "(((uintptr_t)a.small | (uintptr_t)a.w) & 15) != 0", "conv", "dvae_convT4s2_fwd", _T, "off", ("small", 4), _GU),
    _p("launch_up_thin", "conv_thin.hip:695", "((uintptr_t)a.out & 7) != 0", "conv", "dvae_convT4s2_fwd", _T, "off", ("big", 4), "k_up_thin_px<3>"),
    _p("launch_up_thin_recon", "conv_thin.hip:705", "a.small_layout != DVAE_NHWC", "fused", "dvae_convT4s2_sigmoid_recon_fwd", _T, "sl", "NCHW",
       "k_up_generic + k_recon_loss"),
    _unreachable("launch_up_thin_recon", "conv_thin.hip:705", "a.out_layout != DVAE_NCHW",
                 "dvae_convT4s2_sigmoid_recon_fwd (capi.hip:143) builds the arguments with the literal DVAE_NCHW: recon is NCHW by contract"),
    _unreachable("launch_wgrad_thin", "conv_thin.hip:765", "Cb == 1", _CALLER % "run_wgrad (capi.hip:67)"),
    _unreachable("launch_wgrad_thin", "conv_thin.hip:765", "Cb == 3", _CALLER % "run_wgrad (capi.hip:67)"),
    _unreachable("launch_wgrad_thin", "conv_thin.hip:765", "Hs != 32", _CALLER % "run_wgrad (capi.hip:67)"),
    # ---- conv_thin_ws.hip (N >= 192: the pairs are the tests of the wave-specialised switch, which run 193 images)
    _unreachable("launch_down_thin_ws", "conv_thin_ws.hip:326", "a.act != DVAE_ACT_NONE",
                 "mask_bits comes from dvae_convT3_dgrad_bits alone, which passes DVAE_ACT_NONE, no bias and no out_bits (capi.hip:443)"),
    _unreachable("launch_down_thin_ws", "conv_thin_ws.hip:327", "a.act != DVAE_ACT_RELU",
                 "out_bits comes from dvae_conv1_fwd_bits alone, which passes DVAE_ACT_RELU (capi.hip:420)"),
    _p("launch_down_thin_ws", "conv_thin_ws.hip:328", "& 15", "thin_ws", "dvae_conv4s2_fwd", dict(N=193, C=3, off=0), "off", 4, "k_down_thin<3, 0, float>",
       _PAST + "[193-3]", V + "test_thin_ends_past_the_cap_on_buffers_the_wave_specialised_kernels_decline"),
    _p("launch_down_thin_ws", "conv_thin_ws.hip:330", "& 15", "thin_ws", "dvae_conv1_fwd_bits, dvae_convT3_dgrad_bits", dict(N=193, C=3, off=0), "off", 4,
       "k_down_thin<3, 3, float> / k_down_thin<3, 2, float>", _PAST + "[193-3]",
       V + "test_thin_ends_past_the_cap_on_buffers_the_wave_specialised_kernels_decline"),
    _unreachable("launch_wgrad_thin_ws", "conv_thin_ws.hip:625", "Cb != 1", _CALLER % "launch_wgrad_thin (conv_thin.hip:765)"),
    _unreachable("launch_wgrad_thin_ws", "conv_thin_ws.hip:625", "Cb != 3", _CALLER % "launch_wgrad_thin (conv_thin.hip:765)"),
    _p("launch_wgrad_thin_ws", "conv_thin_ws.hip:626", "& 15", "thin_ws", _WG, dict(N=193, C=3, off=0), "off", 4, "k_wgrad_thin<3, float>",
       _PAST + "[193-3]", V + "test_thin_ends_past_the_cap_on_buffers_the_wave_specialised_kernels_decline"),
    # ---- conv_generic.hip: the k_*_thin_px branches
    _p("launch_down_generic", "conv_generic.hip:342", "a.Cs == 32", "conv", _DN, _PX, "Cs", 16, _GD),
    _p("launch_down_generic", "conv_generic.hip:342", "a.Cb == 1", "conv", _DN, _PX1, "Cb", 2, _GD),
    _p("launch_down_generic", "conv_generic.hip:342", "a.Cb == 3", "conv", _DN, _PX, "Cb", 4, _GD),
    _p("launch_down_generic", "conv_generic.hip:342", "a.big_layout == DVAE_NCHW", "conv", _DN, _PX, "bl", "NHWC", _GD),
    _p("launch_down_generic", "conv_generic.hip:342", "a.out_layout == DVAE_NHWC", "conv", _DN, _PX, "sl", "NCHW", _GD),
    _p("launch_down_generic", "conv_generic.hip:343", "& 15", "conv", _DN, _PX, "off", ("small", 4), _GD),
    _p("launch_up_generic", "conv_generic.hip:362", "a.Cs == 32", "conv", _UP, _PX, "Cs", 16, _GU),
    _p("launch_up_generic", "conv_generic.hip:362", "a.Cb == 1", "conv", _UP, _PX1, "Cb", 2, _GU),
    _p("launch_up_generic", "conv_generic.hip:362", "a.Cb == 3", "conv", _UP, _PX, "Cb", 4, _GU),
    _p("launch_up_generic", "conv_generic.hip:362", "a.small_layout == DVAE_NHWC", "conv", _UP, _PX, "sl", "NCHW", _GU),
    _p("launch_up_generic", "conv_generic.hip:362", "& 15", "conv", _UP, _PX, "off", ("small", 8), _GU),
    # ---- linear.hip (through the C-ABI lda = ldb = K forward, lda = N and ldb = K for the input gradient: one argument moves both)
    _p("try_fc32", "linear.hip:414", "& 15", "linear", _FW, _L, "off", ("x", 4), "k_gemm<true, false>"),
    _p("try_fc32<false>", "linear.hip:415", "Kc % 4", "linear", _FW, _L12, "K", 10, "k_fc32<32, false, 1>"),
    _p("try_fc32<false>", "linear.hip:415", "lda % 4", "linear", _FW, _L12, "K", 10, "k_fc32<32, false, 1>"),
    _p("try_fc32<false>", "linear.hip:415", "ldb % 4", "linear", _FW, _L12, "K", 10, "k_fc32<32, false, 1>"),
    _p("try_fc32", "linear.hip:419", "Kc % 4", "linear", _FW, _L, "K", 510, "k_gemm<true, false>"),
    _p("try_fc32<true>", "linear.hip:419", "lda % 4", "linear", _DG, _L, "N", 255, "k_gemm<true, true>"),
    _p("try_fc32<true>", "linear.hip:420", "N % 4", "linear", _DG, _L12, "K", 10, "k_fc32<256, true, 2>"),
    _p("try_fc32<true>", "linear.hip:420", "ldb % 4", "linear", _DG, _L12, "K", 10, "k_fc32<256, true, 2>"),
    _unreachable("try_fc32<false>", "linear.hip:421", "ldb % 4", "the forward passes ldb = K = Kc, and linear.hip:419 has already returned for Kc % 4 != 0"),
    _p("try_fcw32", "linear.hip:534", "N % 4", "linear", _WGL, _L, "N", 255, "k_gemm<false, true>"),
    _p("try_fcw32", "linear.hip:534", "K % 4", "linear", _WGL, _L, "K", 510, "k_gemm<false, true>"),
    _p("try_fcw32", "linear.hip:535", "& 15", "linear", _WGL, _L, "off", ("dy", 8), "k_gemm<false, true>"),
    _p("launch_linear_fwd", "linear.hip:629", "K % 4 == 0", "linear", _FW, _LS, "K", 1001, "k_gemm<true, false> + k_splitk_epilogue"),
    _p("launch_linear_fwd", "linear.hip:629", "& 15", "linear", _FW, _LS, "off", ("w", 4), "k_gemm<true, false> + k_splitk_epilogue"),
    _unreachable("launch_linear_dgrad", "linear.hip:670", "N % 4 == 0", _SMALL_ONLY),
    _unreachable("launch_linear_dgrad", "linear.hip:670", "& 15", _SMALL_ONLY),
    # ---- gemm_dma.hip
    _p("launch_gdma_t (vec_ok)", "gemm_dma.hip:473", "N % 4 == 0", "linear", _FW, _LD, "N", 1002, "k_gdma<32, 32, 64, 3, 4, false, 0> (scalar epilogue)"),
    _p("launch_gdma_t (vec_ok)", "gemm_dma.hip:473", "ldc % 4 == 0", "linear", _FW, _LD, "N", 1002, "k_gdma<32, 32, 64, 3, 4, false, 0> (scalar epilogue)"),
    _p("launch_gdma_t (vec_ok)", "gemm_dma.hip:473", "& 15", "linear", _FW, _LD, "off", ("y", 4), "k_gdma<32, 32, 64, 3, 4, false, 0> (scalar epilogue)"),
    _p("try_gdma", "gemm_dma.hip:482", "Kc % 4", "linear", _FW, _LD, "K", 1001, "k_gemm<true, false>"),
    _p("try_gdma", "gemm_dma.hip:482", "lda % 4", "linear", _DG, _LD, "N", 1001, "k_gemm<true, true>"),
    _p("try_gdma", "gemm_dma.hip:482", "ldb % 4", "linear", _FW, _LD, "K", 1001, "k_gemm<true, false>"),
    _p("try_gdma", "gemm_dma.hip:482", "N % 4", "linear", _DG, _LD, "K", 1001, "k_gemm<true, true>"),
    _p("try_gdma", "gemm_dma.hip:483", "& 15", "linear", _FW, _LD, "off", ("w", 4), "k_gemm<true, false>"),
    _p("try_gdma_wgrad", "gemm_dma.hip:517", "N % 4", "linear", _WGL, _LD, "N", 1002, "k_gemm<false, true>"),
    _p("try_gdma_wgrad", "gemm_dma.hip:517", "K % 4", "linear", _WGL, _LD, "K", 1001, "k_gemm<false, true>"),
    _p("try_gdma_wgrad", "gemm_dma.hip:519", "& 15", "linear", _WGL, _LD, "off", ("dw", 8), "k_fcw32<64>"),
    # ---- linear_narrow.hip
    _p("try_narrow_fwd", "linear_narrow.hip:88", "K % 4", "linear", _FW, _LN, "K", 1001, "k_gemm<true, false>"),
    _p("try_narrow_fwd", "linear_narrow.hip:88", "aligned16(x, w)", "linear", _FW, _LN, "off", ("x", 4), "k_gemm<true, false>"),
    _p("try_narrow_dgrad", "linear_narrow.hip:99", "K % 4", "linear", _DG, _LN, "K", 1001, "k_gemm<true, true>"),
    _p("try_narrow_dgrad", "linear_narrow.hip:99", "aligned16(w, x_act, dx)", "linear", _DG, _LN, "off", ("dx", 4), "k_gemm<true, true>"),
    # ---- linear_grouped.hip: the two flag bits of a problem (each problem of one launch of test_linear_wgrad_grouped_flag_bits)
    _p("launch_linear_wgrad_grouped", "linear_grouped.hip:161", "p.N % 4 == 0", "grouped", "dvae_linear_wgrad_grouped", dict(_GRP, K=256), "N", 18,
       "k_fcw_grouped<64>, 4-byte loads of dy", _GRP_BASE, _GRP_TEST),
    _p("launch_linear_wgrad_grouped", "linear_grouped.hip:161", "((uintptr_t)p.dy & 15) == 0", "grouped", "dvae_linear_wgrad_grouped", dict(_GRP, K=256, N=20),
       "dy_off", 4, "k_fcw_grouped<64>, 4-byte loads of dy", _GRP_BASE, _GRP_TEST),
    _p("launch_linear_wgrad_grouped", "linear_grouped.hip:161", "p.K % 4 == 0", "grouped", "dvae_linear_wgrad_grouped", dict(_GRP, K=12), "K", 10,
       "k_fcw_grouped<64>, 4-byte loads of x", _GRP_BASE, _GRP_TEST),
    _p("launch_linear_wgrad_grouped", "linear_grouped.hip:161", "((uintptr_t)p.x & 15) == 0", "grouped", "dvae_linear_wgrad_grouped", dict(_GRP, K=256, N=20),
       "x_off", 8, "k_fcw_grouped<64>, 4-byte loads of x", _GRP_BASE, _GRP_TEST),
]

# The launcher-condition lines the host test scans for ==, !=, % and alignment comparisons: every comparison found on them must
# be the `term` of a row above with that `where` -- a term added to one of these conditions later fails the host test until it
# has its pair.  (file, lines)
PREDICATE_LINES = [
    ("capi.hip", (31, 42, 57, 58, 60, 61, 63, 64, 67, 142, 145)),
    ("conv_mfma.hip", (439, 440, 445, 447, 449, 455, 457, 468)),
    ("conv_up_ws.hip", (382, 383, 385)),
    ("conv_thin.hip", (671, 675, 676, 694, 695, 705, 765)),
    ("conv_thin_ws.hip", (326, 327, 328, 330, 625, 626)),
    ("conv_generic.hip", (342, 343, 362)),
    ("linear.hip", (414, 415, 419, 420, 421, 534, 535, 629, 670)),
    ("gemm_dma.hip", (473, 482, 483, 517, 519)),
    ("linear_narrow.hip", (88, 99)),
    ("linear_grouped.hip", (161,)),
]
