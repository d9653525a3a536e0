# TEST-ONLY sanitizer build (CPU; a stand-alone program with its own main, never loaded into python):
#   essential_plan_harness : the planner of OptimizeEssentialGraph (orbslam2_amd/csrc/orbfe_essential_plan.cpp) under ASan + UBSan
CXX      ?= g++
SAN      = -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fno-fast-math
CSRC     = ../../orbslam2_amd/csrc
all: essential_plan_harness
essential_plan_harness: essential_plan_harness.cpp $(CSRC)/orbfe_essential_plan.cpp ../../include/orbfe.h essential_plan.mk
	$(CXX) $(CXXFLAGS) $(SAN) -o $@ essential_plan_harness.cpp $(CSRC)/orbfe_essential_plan.cpp
clean:
	rm -f essential_plan_harness
