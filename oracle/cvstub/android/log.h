// Stand-in for <android/log.h>, written for oracle/Makefile.ref: the reference's DBoW2 logs through __android_log_print; here the
// call does nothing.  TEST INFRASTRUCTURE ONLY.
#ifndef ORACLE_CVSTUB_ANDROID_LOG_H
#define ORACLE_CVSTUB_ANDROID_LOG_H

enum { ANDROID_LOG_VERBOSE = 2, ANDROID_LOG_INFO = 4, ANDROID_LOG_ERROR = 6 };   // VERBOSE: ORBextractor.cc (orb_ref_harness)

static inline int __android_log_print(int, const char*, const char*, ...) { return 0; }

#endif
