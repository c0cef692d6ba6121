// How csrc/jpeg_entropy.cpp, which builds without the rest of the library, reports the cause of a refusal: the text is
// kept per thread, and handed to `jpeg_error_sink` when one is set (jpeg_host.cpp routes it into ilcc_last_error).
#ifndef ILCC_JPEG_ENTROPY_H_
#define ILCC_JPEG_ENTROPY_H_

namespace ilcc {
extern void (*jpeg_error_sink)(const char*);
const char* jpeg_last_error();
}  // namespace ilcc

#endif
