// What the stand-alone programs of this directory check with: a failed CHECK is printed and counted and the program goes on; main returns 1
// where `failures` is not zero, before it prints its "clean" line.
#pragma once
#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)
