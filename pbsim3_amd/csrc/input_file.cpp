// input_file.cpp -- open_input (input_file.h): gzip inputs inflated into an anonymous mapping, BGZF on the GPU
// (inflate_host.cpp), other gzip through zlib on the host; a plain file, a pipe or a file that cannot be opened is not
// touched here, so its reader goes on exactly as before.
#include "input_file.h"

#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <vector>

#include "../../include/pbsim3_amd.h"
#include "inflate_host.h"

namespace pbsim {

namespace {
thread_local pbsim_ctx *t_ctx = nullptr;

struct Map {  // the file, read-only
  void *p = MAP_FAILED;
  size_t n = 0;
  ~Map() {
    if (p != MAP_FAILED) munmap(p, n);
  }
};

bool anon(size_t n, InputBytes *in) {
  in->size = n;
  if (n == 0) return true;
  void *p = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (p == MAP_FAILED) return false;
  in->map = p;
  return true;
}

// concatenated gzip members through zlib, to the end of the file, straight into an anonymous mapping that grows as needed
// (and is cut to size at the end); anything after the last member is an error
bool zlib_inflate(const char *file, const uint8_t *src, size_t n, InputBytes *in, std::string *err) {
  size_t cap = std::max<size_t>(n * 4, 1u << 20), used = 0;
  uint8_t *out = (uint8_t *)mmap(nullptr, cap, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (out == (uint8_t *)MAP_FAILED) {
    *err = std::string(file) + ": no memory for the inflated bytes";
    return false;
  }
  auto give_up = [&](const std::string &m) {
    munmap(out, cap);
    *err = std::string(file) + ": " + m;
    return false;
  };
  size_t off = 0;
  while (off < n) {
    if (n - off < 2 || src[off] != 0x1f || src[off + 1] != 0x8b)
      return give_up("bytes after the last gzip member at byte offset " + std::to_string(off));
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) return give_up("zlib: inflateInit2 failed");
    size_t pos = off;
    const std::string where = "gzip member at byte offset " + std::to_string(off) + ": ";
    for (;;) {
      if (z.avail_in == 0 && pos < n) {
        z.next_in = const_cast<Bytef *>(src + pos);
        z.avail_in = (uInt)std::min<size_t>(n - pos, 1u << 30);
        pos += z.avail_in;
      }
      if (cap - used < (1u << 20)) {
        void *p = mremap(out, cap, cap * 2, MREMAP_MAYMOVE);
        if (p == MAP_FAILED) {
          inflateEnd(&z);
          return give_up("no memory for the inflated bytes");
        }
        out = (uint8_t *)p;
        cap *= 2;
      }
      z.next_out = out + used;
      z.avail_out = (uInt)std::min<size_t>(cap - used, 1u << 30);
      const uInt room = z.avail_out;
      const int rc = inflate(&z, Z_NO_FLUSH);
      used += room - z.avail_out;
      if (rc == Z_STREAM_END) break;
      if (rc != Z_OK && rc != Z_BUF_ERROR) {
        const std::string m = z.msg ? z.msg : "invalid data";
        inflateEnd(&z);
        return give_up(where + m);
      }
      if (z.avail_in == 0 && pos == n && z.avail_out != 0) {
        inflateEnd(&z);
        return give_up(where + "unexpected end of file");
      }
    }
    off = pos - z.avail_in;
    inflateEnd(&z);
  }
  if (used == 0) {
    munmap(out, cap);
    in->size = 0;
    return true;
  }
  void *p = mremap(out, cap, used, 0);  // shrinking in place
  if (p == MAP_FAILED) return give_up("cannot trim the inflated bytes");
  in->map = p;
  in->size = used;
  return true;
}
}  // namespace

pbsim_ctx *set_input_context(pbsim_ctx *ctx) {
  pbsim_ctx *was = t_ctx;
  t_ctx = ctx;
  return was;
}

int open_input(const char *file, InputBytes *in, std::string *err) {
  struct stat sb;
  if (stat(file, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 2) return 0;  // (a FIFO is never opened here)
  const int fd = open(file, O_RDONLY);
  if (fd < 0) return 0;
  unsigned char magic[2];
  if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 2 || pread(fd, magic, 2, 0) != 2 || magic[0] != 0x1f ||
      magic[1] != 0x8b) {
    close(fd);
    return 0;
  }
  Map m;
  m.n = (size_t)sb.st_size;
  m.p = mmap(nullptr, m.n, PROT_READ, MAP_PRIVATE, fd, 0);
  close(fd);
  if (m.p == MAP_FAILED) {
    *err = std::string(file) + ": cannot map the gzip file";
    return -1;
  }
  (void)madvise(m.p, m.n, MADV_SEQUENTIAL);
  const uint8_t *src = (const uint8_t *)m.p;
  std::vector<BgzfMember> mem;
  if (!bgzf_index(src, (int64_t)m.n, &mem)) return zlib_inflate(file, src, m.n, in, err) ? 1 : -1;
  // BGZF: every member at once on the GPU
  if (!t_ctx) {
    *err = std::string(file) + ": a BGZF input needs the GPU context to inflate it";
    return -1;
  }
  if (!anon((size_t)bgzf_inflated_size(mem), in)) {
    *err = std::string(file) + ": no memory for the inflated bytes";
    return -1;
  }
  if (!inflate_members(t_ctx, src, mem, (uint8_t *)in->map)) {
    *err = std::string(file) + ": " + pbsim_last_error();
    return -1;
  }
  return 1;
}

}  // namespace pbsim
