// The image-transform kernels' launchers that another translation unit calls (image.hip defines them; diag.hip's mb_image_coeffs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mb {

constexpr int IMG_MAX_SIDE = 16384;      // source and resized sides
constexpr int IMG_MAX_JOBS = 4096;       // jobs of one pass (a grid dimension)
constexpr int IMG_BOX = 0, IMG_BILINEAR = 1, IMG_BICUBIC = 2;

// taps per output of one axis: Pillow's ksize, or 1 for an axis whose size does not change (the identity table)
int image_ksize(int in_size, int out_size, int filter);
// the table of outputs [first, first + count) of one axis on caller-owned arrays: xmin [count], n [count], taps [count][ksize] (zero beyond n)
void image_coeffs_launch(int in_size, int out_size, int filter, int first, int count, int ksize, int32_t* xmin, int32_t* n, int32_t* taps, hipStream_t s);

}  // namespace mb
