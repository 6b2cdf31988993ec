!==========================================================================!
! matmat_test_hip: multi-vector products through the stand-alone host      !
! layer.  The 5-point matrix of a 37 x 29 grid times a block of 7 columns  !
! (hip_matmat, hip_matmat_add, hip_matmat_t, hip_matmat_t_add); every      !
! column is compared with the single-vector product of that column with    !
! `==`: the contract of sgm_mat_matmat (include/sigma_hip.h).              !
!==========================================================================!
program matmat_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx = 37, ny = 29, n = nx * ny, k = 7
    type(hip_csr_matrix), target :: A
    real(dp), allocatable :: X(:,:), Y(:,:), Y0(:,:), y1(:)
    integer :: i, j, fails
    logical :: same

    fails = 0
    call hip_check(sgm_init(0_c_int))
    call grid5(A)
    allocate(X(n, k), Y(n, k), Y0(n, k), y1(n))
    do j = 1, k
        do i = 1, n
            X(i, j) = sin(0.37_dp * i + 1.3_dp * j) + 0.01_dp * j
            Y0(i, j) = cos(0.11_dp * i - 0.7_dp * j)
        enddo
    enddo

    Y = -1.0_dp
    call A%matmat(X, Y)
    same = .true.
    do j = 1, k
        call A%matvec(X(:, j), y1)
        same = same .and. all(Y(:, j) == y1)
    enddo
    call check('matmat: every column == matvec of that column', same)

    Y = Y0
    call A%matmat_add(X, Y)
    same = .true.
    do j = 1, k
        y1 = Y0(:, j)
        call A%matvec_add(X(:, j), y1)
        same = same .and. all(Y(:, j) == y1)
    enddo
    call check('matmat_add: every column == matvec_add of that column', same)

    Y = -1.0_dp
    call A%matmat_t(X, Y)
    same = .true.
    do j = 1, k
        call A%matvec_t(X(:, j), y1)
        same = same .and. all(Y(:, j) == y1)
    enddo
    call check('matmat_t: every column == matvec_t of that column', same)

    Y = Y0
    call A%matmat_t_add(X, Y)
    same = .true.
    do j = 1, k
        y1 = Y0(:, j)
        call A%matvec_t_add(X(:, j), y1)
        same = same .and. all(Y(:, j) == y1)
    enddo
    call check('matmat_t_add: every column == matvec_t_add of that column', same)

    call A%destroy()
    if (fails > 0) then
        print *, 'matmat_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'matmat_test_hip: ok'

contains

subroutine grid5(M)
    ! the 5-point matrix of the nx x ny grid, columns ascending; values that differ from entry to entry
    type(hip_csr_matrix), intent(inout) :: M
    integer :: ptr(n + 1), node(5 * n), r, ix, iy, e, s, c
    integer, parameter :: off(5) = [-nx, -1, 0, 1, nx]
    real(dp) :: val(5 * n)
    logical :: inside
    e = 0
    do r = 1, n
        ix = mod(r - 1, nx); iy = (r - 1) / nx
        ptr(r) = e + 1
        do s = 1, 5
            inside = .true.
            if (s == 1) inside = iy > 0
            if (s == 2) inside = ix > 0
            if (s == 4) inside = ix < nx - 1
            if (s == 5) inside = iy < ny - 1
            if (.not. inside) cycle
            c = r + off(s)
            e = e + 1
            node(e) = c
            val(e) = merge(4.0_dp, -1.0_dp, s == 3) + 0.001_dp * mod(e, 17)
        enddo
    enddo
    ptr(n + 1) = e + 1
    call M%init(n, n, ptr, node(1:e))
    M%val = val(1:e)
    M%values_dirty = .true.
end subroutine

subroutine check(what, ok)
    character(len=*), intent(in) :: what
    logical, intent(in) :: ok
    if (ok) then
        print *, 'ok    ', what
    else
        print *, 'FAILED ', what
        fails = fails + 1
    endif
end subroutine

end program matmat_test_hip
