// Host stand-in for ntjoin_amd/csrc/bisect.h, for tools/nthash_check.cpp only: nthash_dev.h's find_run and run_of_kmer are calls
// of the one header, which stays where it is.  This directory is copied before it is used (tests/test_nthash_cpu.py), so the path
// below is not relative to this file: it resolves through the -I <repository>/include of that build.
#pragma once
#include "../ntjoin_amd/csrc/bisect.h"
