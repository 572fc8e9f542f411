// handoff.h -- the next-up descriptor of the job pipeline's lane hand-off (job.cpp): the main loop publishes the
// round whose text emission it has just enqueued; each of the two delivery lanes of the round in front takes it once, at its
// tail, and launches the head of the next round's compression; the main loop withdraws it before the round's own delivery
// starts (or before the slot's text is written again).  Plain C++ (no HIP): tests/handoff_tsan_main.cpp runs it under
// -fsanitize=thread.
#pragma once
#include <stdint.h>

#include <mutex>

namespace pbsim {

struct HandoffNext {
  int slot = -1;
  const void *text[2] = {nullptr, nullptr};  // read | MAF text of the slot (device)
  int64_t bytes[2] = {0, 0};
  void *ev_text = nullptr;                   // behind the text emission
};

class Handoff {
 public:
  // main loop: the descriptor is up from here on (one at a time: a descriptor still up is replaced)
  void publish(const HandoffNext &d) {
    std::lock_guard<std::mutex> lk(mu_);
    d_ = d;
    up_ = true;
    taken_[0] = taken_[1] = false;
  }
  // lane `lane` (0 | 1), on its own thread: run(descriptor) once per lane and descriptor, under the lock -- withdraw()
  // returns only when no run() is in progress, and what run() wrote is visible to whoever withdrew.
  // false: no descriptor is up yet (ask again later); true: taken now or before.
  template <class F>
  bool take(int lane, F &&run) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!up_) return false;
    if (!taken_[lane]) {
      taken_[lane] = true;
      run(d_);
    }
    return true;
  }
  // main loop: nobody takes the descriptor from here on.  Bit `lane` of the result: that lane had taken it.
  unsigned withdraw() {
    std::lock_guard<std::mutex> lk(mu_);
    const unsigned t = up_ ? (unsigned)taken_[0] | ((unsigned)taken_[1] << 1) : 0u;
    up_ = false;
    taken_[0] = taken_[1] = false;
    return t;
  }

 private:
  std::mutex mu_;
  bool up_ = false;
  bool taken_[2] = {false, false};
  HandoffNext d_;
};

}  // namespace pbsim
