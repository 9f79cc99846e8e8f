/* Stand-in for the reference's Optimizer.h for oracle/_ref/libos1_initializer.so: src/Initializer.cc includes it and uses nothing of
 * it.  Our own text.  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_INITIALIZER_DECL_OPTIMIZER_H_
#define OS1_INITIALIZER_DECL_OPTIMIZER_H_
#endif
