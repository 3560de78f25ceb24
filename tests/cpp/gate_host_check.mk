# Builds gate_host_check: icp4r_sequence_pairs' host code alone (csrc/icp4r_gate_pairs.hpp), under the
# host sanitizers — a stand-alone program, no library.  make -C tests/cpp -f gate_host_check.mk
ROOT := $(abspath ../..)
OUT := $(ROOT)/tests/cpp/_build

all: $(OUT)/gate_host_check

$(OUT)/gate_host_check: gate_host_check.cpp $(ROOT)/icp-4dradar_amd/csrc/icp4r_gate_pairs.hpp
	@mkdir -p $(OUT)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/icp-4dradar_amd/csrc -o $@ gate_host_check.cpp

.PHONY: all
