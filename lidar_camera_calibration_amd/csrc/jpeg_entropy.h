// How csrc/jpeg_entropy.cpp, which builds without the rest of the library, reports the cause of a refusal: the text is
// kept per thread, and handed to `jpeg_error_sink` when one is set (jpeg_host.cpp routes it into ilcc_last_error).
#ifndef ILCC_JPEG_ENTROPY_H_
#define ILCC_JPEG_ENTROPY_H_

#include <cstdint>

#include "ilcc_jpeg.h"

namespace ilcc {
extern void (*jpeg_error_sink)(const char*);
const char* jpeg_last_error();
// records "jpeg: cause (detail)" as the thread's text, hands it to the sink and returns ILCC_BAD_ARGUMENT; the encoder
// (csrc/jpeg_entropy_enc.cpp) refuses through it too
int32_t jpeg_refuse(const char* cause, const char* detail = nullptr);
// true when the info's sizes, sampling, block counts and offsets are the ones ilcc_jpeg_layout gives: what K13, K14 and the
// encoder ask of an info before they index with it
bool jpeg_laid_out(const ilcc_jpeg_info& info);
}  // namespace ilcc

#endif
