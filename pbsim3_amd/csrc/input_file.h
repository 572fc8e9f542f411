// input_file.h -- the one way the input readers open a file (input_file.cpp): a gzip file, recognised by its first two
// bytes, is handed back inflated -- BGZF on the GPU of the calling thread's context, any other gzip through zlib on the
// host --, and everything else is left to the reader's own code, unchanged.
#pragma once
#include <stddef.h>
#include <sys/mman.h>

#include <string>

struct pbsim_ctx;

namespace pbsim {

struct InputBytes {  // the inflated bytes of a gzip input: an anonymous mapping of exactly `size` bytes
  void *map = nullptr;
  size_t size = 0;
  InputBytes() = default;
  InputBytes(const InputBytes &) = delete;
  InputBytes &operator=(const InputBytes &) = delete;
  ~InputBytes() {
    if (map) munmap(map, size);
  }
};

// 1: `file` is a regular file holding gzip, *in has its inflated bytes; 0: it is not (or cannot be opened) -- read it as
// before; -1: a gzip file that does not inflate, *err = "<file>: gzip member at byte offset N: <reason>" (or as fitting).
// Declared weak: the readers (unit_io.cpp) also build without the library (the host sanitizer drivers), where every
// file is then read as before.
int open_input(const char *file, InputBytes *in, std::string *err) __attribute__((weak));
// the context whose GPU inflates BGZF inputs opened on the calling thread (each rank thread sets its own; nullptr: none);
// returns the one set before
pbsim_ctx *set_input_context(pbsim_ctx *ctx) __attribute__((weak));

}  // namespace pbsim
