# Builds vgicp_callsite: a fast_gicp FastVGICP block written against include/icp4r/fast_gicp_compat.hpp and
# libicp4r.so.  make -C tests/cpp -f vgicp_callsite.mk
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/icp-4dradar_amd/icp4r/_lib
OUT := $(ROOT)/tests/cpp/_build

all: $(OUT)/vgicp_callsite

$(OUT)/vgicp_callsite: vgicp_callsite.cpp $(ROOT)/include/icp4r/fast_gicp_compat.hpp $(ROOT)/include/icp4r/pcl_compat.hpp \
                       $(ROOT)/include/icp4r/icp4r_gicp.h $(ROOT)/include/icp4r/icp4r_vgicp.h $(LIBDIR)/libicp4r.so
	@mkdir -p $(OUT)
	g++ -O2 -std=c++17 -Wall -I$(ROOT)/include -o $@ vgicp_callsite.cpp -L$(LIBDIR) -licp4r -Wl,-rpath,$(LIBDIR)

.PHONY: all
