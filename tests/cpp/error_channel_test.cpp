// tests/cpp/error_channel_test.cpp -- the one error string behind klstm_last_error().  Three entries that live in three translation
// units of the library (klstm_set_option: klstm_engine.hip; klstm_ctc_eval: klstm_api_ctc.hip; klstm_reverse_streams:
// klstm_api_ops.hip) fail their argument checks, which fire before any HIP call: no device is needed.  Each message must be readable
// through klstm_last_error(), the last one must win, and a thread that has made no call must read an empty string while the first
// thread's message stays in place: one thread_local string for the library, not one per translation unit.  tests/test_abi.py runs it.
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "klstm.h"

static int failures = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) { std::printf("FAILED %s:%d: %s (last error: '%s')\n", __FILE__, __LINE__, #c, klstm_last_error()); failures++; } \
  } while (0)

int main() {
  CHECK(std::strcmp(klstm_last_error(), "") == 0);

  CHECK(klstm_set_option(nullptr, "graph", 0) == KLSTM_ERR_ARG);
  CHECK(std::strcmp(klstm_last_error(), "null argument") == 0);

  float x = 0.f;
  int n = 0;
  CHECK(klstm_ctc_eval(&x, /*T*/ 0, 1, 4, 4, &n, &n, &n, 0, &x, 4, &x, nullptr, &x, 0, nullptr) == KLSTM_ERR_ARG);
  CHECK(std::strncmp(klstm_last_error(), "klstm_ctc_eval: bad size", 24) == 0);

  CHECK(klstm_reverse_streams(&x, 1, 1, 1, 1, &n, &x, 1, /*mode*/ 99, nullptr) == KLSTM_ERR_ARG);
  CHECK(std::strstr(klstm_last_error(), "unknown mode 99") != nullptr);
  CHECK(std::strcmp(klstm_last_error(), "klstm_reverse_streams: unknown mode 99") == 0);

  std::string other = "unread";
  std::thread t([&] { other = klstm_last_error(); });
  t.join();
  CHECK(other.empty());
  CHECK(std::strcmp(klstm_last_error(), "klstm_reverse_streams: unknown mode 99") == 0);   // still in place in this thread

  // and the other way round: a failure on another thread leaves this thread's string alone
  std::thread u([&] {
    (void)klstm_set_option(nullptr, "graph", 0);
    other = klstm_last_error();
  });
  u.join();
  CHECK(other == "null argument");
  CHECK(std::strcmp(klstm_last_error(), "klstm_reverse_streams: unknown mode 99") == 0);

  if (failures) return 1;
  std::printf("OK error channel: 3 translation units, 1 string per thread\n");
  return 0;
}
