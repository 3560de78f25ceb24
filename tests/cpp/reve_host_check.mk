# Builds reve_host_check: the host arithmetic of the 3D Doppler ego-velocity estimator alone
# (csrc/icp4r_reve_math.hpp), under the host sanitizers — a stand-alone program, no library.
# make -C tests/cpp -f reve_host_check.mk
ROOT := $(abspath ../..)
OUT := $(ROOT)/tests/cpp/_build

all: $(OUT)/reve_host_check

$(OUT)/reve_host_check: reve_host_check.cpp $(ROOT)/icp-4dradar_amd/csrc/icp4r_reve_math.hpp
	@mkdir -p $(OUT)
	g++ -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -fno-omit-frame-pointer -I$(ROOT)/icp-4dradar_amd/csrc -o $@ reve_host_check.cpp

.PHONY: all
