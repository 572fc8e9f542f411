// hp_census_weighted (host_tables.cpp) with weight 1 over every line of a file: twelve counts per line.
// usage: hp_census_driver <keep_first_case 0|1> <file of units, one per line>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "host_tables.h"
using namespace pbsim;
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const int keep_first = atoi(argv[1]);
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  std::vector<uint8_t> unit;
  for (int ch; (ch = fgetc(f)) != EOF;) {
    if (ch != '\n') {
      unit.push_back((uint8_t)ch);
      continue;
    }
    int64_t freq[kHpSlots] = {0};
    if (!unit.empty()) hp_census_weighted(unit.data(), (int64_t)unit.size(), 1, keep_first, freq);
    for (int v = 0; v < kHpSlots; v++) printf("%lld%c", (long long)freq[v], v + 1 < kHpSlots ? ' ' : '\n');
    unit.clear();
  }
  fclose(f);
  return 0;
}
