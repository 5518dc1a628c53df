// Test-only stand-in for <gtextutils/container_join.h>, written for this project: fastx_uncollapser.cpp includes it and, outside an #if 0, uses nothing of it.
#ifndef FXG_TEST_COMPAT_UC_CONTAINER_JOIN_H
#define FXG_TEST_COMPAT_UC_CONTAINER_JOIN_H
#endif
