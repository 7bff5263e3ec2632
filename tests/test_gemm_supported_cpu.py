"""Host-only: the shapes the half-tile GEMM kernel takes.  Its DMA plan holds 32-bit BYTE offsets into A and W, so gemm_ht_supported must refuse every
shape whose M * K * 2 or N * K * 2 reaches 2^32 (the launcher then falls back to the 128 x 128 kernel) and accept the shape just below the bound."""
import pytest


def _lib():
    from maskbit_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_half_tile_kernel_refuses_shapes_at_the_32_bit_byte_offset_bound(epi):
    lib = _lib()
    K = 4096
    rows = (1 << 32) // (2 * K)                                                # rows * K * 2 == 2^32 exactly
    assert lib.mb_gemm_ht_supported(epi, rows, 256, K) == 0                    # A: M * K * 2 at the bound
    assert lib.mb_gemm_ht_supported(epi, rows - 1, 256, K) == 1                # one row below it (M * N * 4 = 2^29: far from its own bound)
    assert lib.mb_gemm_ht_supported(epi, 512, rows, K) == 0                    # W: N * K * 2 at the bound
    assert lib.mb_gemm_ht_supported(epi, 512, rows - 256, K) == 1              # one 256-column tile below it
    assert lib.mb_gemm_ht_supported(epi, 1024, 1024, 1024) == 1 and lib.mb_gemm_ht_supported(epi, 1024, 1024, 64) == 0   # (the other rules still hold)
