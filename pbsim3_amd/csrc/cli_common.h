// cli_common.h -- what the simulator's command line (cli.cpp) and the stand-alone modes (cli_stages.cpp) both need: how the
// process ends on an error, and a read-only mapping of an input file.
#pragma once
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {
namespace cli {

// the reference's exit(-1).  Other ranks of the process may be inside HIP calls on their own threads: leave without running
// static destructors under them (everything buffered is flushed first)
[[noreturn]] inline void quit(int status) {
  fflush(NULL);
  _exit(status & 255);
}

[[noreturn]] inline void die(const char *fmt, const char *a = "", const char *b = "") {
  fprintf(stderr, "ERROR");
  fprintf(stderr, fmt, a, b);
  fprintf(stderr, "\n");
  quit(-1);
}

inline void check(int ok) {
  if (!ok) {
    // a rank that only learnt of another rank's failure lets that rank report first (they share this process's stderr and exit)
    if (!strncmp(pbsim_last_error(), "another rank", 12)) usleep(300000);
    fprintf(stderr, "ERROR: %s\n", pbsim_last_error());
    quit(-1);
  }
}

struct MappedFile {
  void *map = MAP_FAILED;
  size_t n = 0;
  ~MappedFile() {
    if (map != MAP_FAILED) munmap(map, n);
  }
  bool open_file(const std::string &name) {
    const int fd = open(name.c_str(), O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size <= 0) {
      if (fd >= 0) close(fd);
      return false;
    }
    n = (size_t)sb.st_size;
    map = mmap(NULL, n, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED) return false;
    (void)madvise(map, n, MADV_SEQUENTIAL);
    return true;
  }
};

}  // namespace cli
}  // namespace pbsim
