// tests/hostlogic/plan_check.cpp -- TEST HARNESS for skch::queryBatchPlan (mashmap_amd/host/skch_types.hpp, no GPU): prints one line per
// environment it tries, for the query file named on the command line:
//   "plan <setting> ctxs <n> batch <bases> pass <bases> buffers <n> bufferBytes <bytes> known <0|1>"
#include <cstdio>
#include <cstdlib>
#include "../../mashmap_amd/host/skch_types.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: plan_check QUERY_FILE\n"); return 2; }
  const char* path = argv[1];
  auto show = [&](const char* what, size_t ctxs) {
    const skch::QueryBatchPlan q = skch::queryBatchPlan({path}, ctxs);
    printf("plan %s ctxs %zu batch %zu pass %zu buffers %zu bufferBytes %zu known %d\n", what, ctxs, q.batchBases, q.passBases, q.buffers, q.bufferBytes, (int)q.inputKnown);
  };
  show("default", 1); show("default", 2);
  setenv("MASHMAP_HIP_COALESCE_MBP", "0", 1); show("coalesce0", 1);
  setenv("MASHMAP_HIP_COALESCE_MBP", "4096", 1); setenv("MASHMAP_HIP_BATCH_MBP", "256", 1); show("b256c4096", 1);
  setenv("MASHMAP_HIP_BATCH_MBP", "0.01", 1); setenv("MASHMAP_HIP_COALESCE_MBP", "2048", 1); show("tiny", 1);
  unsetenv("MASHMAP_HIP_BATCH_MBP"); unsetenv("MASHMAP_HIP_COALESCE_MBP");
  setenv("MASHMAP_HIP_ASCII_UPLOAD", "1", 1); show("ascii", 1); unsetenv("MASHMAP_HIP_ASCII_UPLOAD");
  return 0;
}

