# Builds reve_callsite: the node's ego-velocity step written against include/icp4r/reve_compat.hpp and
# libicp4r.so.  make -C tests/cpp -f reve_callsite.mk
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/icp-4dradar_amd/icp4r/_lib
OUT := $(ROOT)/tests/cpp/_build

all: $(OUT)/reve_callsite

$(OUT)/reve_callsite: reve_callsite.cpp $(ROOT)/include/icp4r/reve_compat.hpp $(ROOT)/include/icp4r/pcl_compat.hpp \
                      $(ROOT)/include/icp4r/icp4r_reve.h $(LIBDIR)/libicp4r.so
	@mkdir -p $(OUT)
	g++ -O2 -std=c++17 -Wall -I$(ROOT)/include -o $@ reve_callsite.cpp -L$(LIBDIR) -licp4r -Wl,-rpath,$(LIBDIR)

.PHONY: all
