// Stand-alone check of pbsim3_amd/csrc/handoff.h under -fsanitize=thread (tests/test_job_handoff_host.py builds and runs it).
// It replays the threads of the job pipeline around the next-up descriptor with plain memory in place of the GPU state:
//   main loop    publishes round r + 1, withdraws it, reads what the lanes left in the slot's lane state (plain ints -- the
//                sanitizer reports a race if withdraw() did not order the lanes' writes before the main loop's reads), then
//                starts the round's own two lane threads, which read that state as well
//   lane threads of round r ask for the descriptor over and over ("no descriptor yet" -> ask again), as the tail hook does
// and checks the protocol: a lane takes a descriptor at most once, never after withdraw(), never its own round's.
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "handoff.h"

namespace {
constexpr int kSlots = 4, kRounds = 400;
struct LaneState {  // what deflate_handoff leaves in a DfLane: plain fields
  int pre_round = -1;
  int launches = 0;
};
LaneState state[kSlots][2];
int failures = 0;
std::atomic<int> taken_total{0};
}  // namespace

int main() {
  pbsim::Handoff h;
  std::vector<std::thread> lanes;
  for (int r = 0; r < kRounds; r++) {
    // the lanes of round r - 1 are running (started below); round r's text is "emitted": publish it
    const int slot = r % kSlots;
    pbsim::HandoffNext d;
    d.slot = slot;
    d.bytes[0] = d.bytes[1] = r;  // carries the round number
    if (r % 7 == 3) {             // a clear round that missed: withdrawn, text written again, published again
      h.publish(d);
      const unsigned took = h.withdraw();
      for (int w = 0; w < 2; w++)
        if (took >> w & 1) {
          if (state[slot][w].pre_round != r) failures++;
          state[slot][w].pre_round = -1;  // settled: the main loop may write the lane's state
        }
    }
    if (r % 11 != 5) h.publish(d);  // (now and then the lanes in front finish before anything is up)
    for (std::thread &t : lanes) t.join();  // "wait for the previous round's bytes"
    lanes.clear();
    const unsigned took = h.withdraw();
    if (h.take(0, [](const pbsim::HandoffNext &) { failures++; })) failures++;  // nothing is up after withdraw()
    int pre[2];
    for (int w = 0; w < 2; w++) {
      pre[w] = state[slot][w].pre_round;  // plain read: ordered behind the lane's write by withdraw()
      if (((took >> w) & 1) != (pre[w] == r)) failures++;
      if (r % 5 == 4) {  // a round that is never delivered (behind the cut): settled, no lane call
        state[slot][w].pre_round = -1;
      }
    }
    if (r % 5 == 4) continue;
    for (int w = 0; w < 2; w++)
      lanes.emplace_back([&h, slot, w, r]() {
        LaneState &mine = state[slot][w];
        if (mine.pre_round != r && mine.pre_round != -1) failures++;  // (never another round's head)
        mine.pre_round = -1;                                          // the call consumes its head
        // the call's tail: ask until something is up, a few times at most (the last round finds nothing)
        for (int tries = 0; tries < 50; tries++) {
          const bool up = h.take(w, [&](const pbsim::HandoffNext &nx) {
            if (nx.bytes[0] != r + 1 || nx.slot == slot) failures++;  // the NEXT round, another slot
            LaneState &next = state[nx.slot][w];
            if (next.pre_round != -1) failures++;  // the slot's lane was idle
            next.pre_round = (int)nx.bytes[0];
            next.launches++;
            taken_total++;
          });
          if (up) break;
          std::this_thread::yield();
        }
      });
  }
  for (std::thread &t : lanes) t.join();
  (void)h.withdraw();
  int launches = 0;
  for (auto &s : state)
    for (auto &l : s) launches += l.launches;
  if (launches != taken_total.load()) failures++;
  printf("handoff: %d rounds, %d lane heads taken, %d failures\n", kRounds, launches, failures);
  return failures == 0 && launches > 0 ? 0 : 1;
}
