/* Stand-in for the reference's ORBmatcher.h for oracle/_ref/libos1_initializer.so: src/Initializer.cc includes it and uses nothing
 * of it.  Our own text.  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_INITIALIZER_DECL_ORBMATCHER_H_
#define OS1_INITIALIZER_DECL_ORBMATCHER_H_
#endif
